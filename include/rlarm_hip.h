/*
 * rlarm_hip.h -- C ABI of librlarm_hip.so: the MI355X (gfx950) implementation of the
 * HER-replay + DDPG-update hot path of PiggyCh/RL_arm_under_sparse_reward.
 *
 * The reference has no FFI of its own (pure Python); its seam is the
 * set of duck-typed Python objects wired in ddpg_agent.py:24-53.  Each entry point below
 * names the reference interface it stands in for (file:line relative to the reference
 * root).  The Python mirror of those objects lives in rl_arm_under_sparse_reward_amd/ and
 * binds this header with ctypes; INTEGRATION.md shows the stub a reference maintainer
 * would add.
 *
 * Conventions
 *   - every function returns 0 on success, a negative hp_status otherwise;
 *     hp_last_error() returns a thread-local message for the last failure;
 *   - "host" pointers are caller-owned and only read/written during the call (the
 *     reference's copy-in / copy-out semantics, replay_buffer.py:39-42, her.py:26);
 *   - "dev" pointers are HIP device addresses (e.g. torch.Tensor.data_ptr());
 *   - all kernels are enqueued on the context's stream (hp_ctx_set_stream), so work
 *     is ordered with whatever else the caller enqueues on that stream;
 *   - calls on the handles of one context are serialised by a per-context lock held for the
 *     duration of each call (the reference's per-object locks, replay_buffer.py:29,34,48 and
 *     normalizer.py:22,27,42): a host feeder thread may call hp_buffer_store while another
 *     thread drives hp_agent_train_cycle; the order in which the calls win the lock is the
 *     order of their work on the stream and of their draws from the shared hp_rng.
 *     hp_ctx_synchronize waits outside the lock.
 *   - there is NO CPU fallback: without a gfx950 device hp_ctx_create fails.
 */
#ifndef RLARM_HIP_H
#define RLARM_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version of the STABLE surface declared in this header.  2 (round 4): the diagnostic / test-hook entry points moved to
 * rlarm_hip_debug.h (no stability promise), hp_agent_fused_status is gone (round 3), hp_agent_train_cycle_pinned,
 * hp_peer_set_gate, hp_ctx_pci_bus_id, hp_agent_status were added.  3 (round 5): hp_buffer_sample_dev (device-output fused
 * sampler) was added.  4 (round 6): hp_ctx_get_stream and hp_ctx_borrow_stream / hp_ctx_return_stream were added (a host that hands
 * device outputs to a framework has them written on the framework's stream for that call instead of rebinding the context), and the sampler's throughput modes
 * (hp_buffer_enable_f32_rows, hp_buffer_sample_dev_f32, hp_buffer_sample_dev_fast).  Still 4 (round 7): the training-state entry
 * points (hp_state_*) were added -- purely additive: no existing declaration, structure or behaviour changed, so a host built against
 * the round-6 header runs unchanged on this library.  hp_abi_version() returns the
 * library's value; a host must refuse a library whose version differs from the header it was built against. */
#define HP_ABI_VERSION 4

typedef enum {
    HP_OK = 0,
    HP_ERR_INVALID = -1,   /* bad argument (maps to ValueError in the Python mirror) */
    HP_ERR_EMPTY = -2,     /* sampling an empty buffer (numpy: "ValueError: high <= 0") */
    HP_ERR_HIP = -3,       /* a HIP runtime call failed */
    HP_ERR_NODEVICE = -4,  /* no gfx950 device visible */
    HP_ERR_STATE = -5      /* call sequence error */
} hp_status;

typedef struct hp_ctx hp_ctx;
typedef struct hp_rng hp_rng;
typedef struct hp_buffer hp_buffer;
typedef struct hp_norm hp_norm;
typedef struct hp_agent hp_agent;
typedef struct hp_comm hp_comm;
typedef struct hp_peer hp_peer;
typedef struct hp_rollout hp_rollout;
typedef struct hp_rng_streams hp_rng_streams;

int hp_abi_version(void);
const char *hp_last_error(void);

/* ---- context ---------------------------------------------------------------------- */
int hp_ctx_create(int device_id, hp_ctx **out);
/* stream == NULL selects a stream owned by the context; to run on the legacy default stream (e.g. to be ordered
 * with a framework that uses it) pass hipStreamLegacy, i.e. (void *)1.  A change of stream keeps the context's work in
 * order: the new stream waits (on the device, not the host) for what the context enqueued on the old one. */
int hp_ctx_set_stream(hp_ctx *ctx, void *hip_stream);
/* the stream the context enqueues on right now (its own one unless hp_ctx_set_stream changed it) */
int hp_ctx_get_stream(hp_ctx *ctx, void **hip_stream);
/* A caller's stream for the duration of ONE call sequence, without rebinding the context: between hp_ctx_borrow_stream and
 * hp_ctx_return_stream (same thread; the context's lock is held in between) every launch of the library goes to `hip_stream`
 * (NULL: the null stream, a framework's default), ordered on the device behind what the context's own stream held; the own
 * stream is ordered behind the borrowed stream's work when it is next used.  No host synchronisation.  What
 * replay_buffer.sample_device wraps hp_buffer_sample_dev in, so that torch consumes the outputs in ITS stream's order while a
 * fused learner on the same context keeps its own stream and its cached graphs. */
int hp_ctx_borrow_stream(hp_ctx *ctx, void *hip_stream);
int hp_ctx_return_stream(hp_ctx *ctx);
int hp_ctx_synchronize(hp_ctx *ctx);
int hp_ctx_device_name(hp_ctx *ctx, char *buf, size_t len);
int hp_ctx_pci_bus_id(hp_ctx *ctx, char *buf, size_t len);      /* "0000:05:00.0"; len >= 16 */
void hp_ctx_destroy(hp_ctx *ctx);

/* ---- random stream ------------------------------------------------------------------
 * Device-resident twin of numpy's legacy global RandomState, which the reference draws
 * from at her.py:24,25,29,31 and replay_buffer.py:64,67 (seeded at train.py:36).
 * State is interoperable with np.random.get_state()/set_state(): (key[624], pos). */
int hp_rng_create(hp_ctx *ctx, hp_rng **out);
int hp_rng_seed(hp_rng *rng, uint32_t seed);                              /* np.random.seed(int) */
int hp_rng_set_state(hp_rng *rng, const uint32_t *key624, int32_t pos);   /* np.random.set_state */
int hp_rng_get_state(hp_rng *rng, uint32_t *key624, int32_t *pos);        /* synchronises */
/* test hooks: the primitive draws, results copied to host (synchronises) */
int hp_rng_randint(hp_rng *rng, int64_t low, int64_t high, int64_t count, int64_t *host_out);
int hp_rng_uniform(hp_rng *rng, int64_t count, double *host_out);
/* ... and the two other primitive draws of the exploration noise (ddpg_agent.py:174-184), in numpy's legacy form: randn(count)
 * (polar method with its cached second normal) and binomial(1, p, count) (inversion; qn = exp(log(1 - p')) with p' = p for
 * p <= 0.5, 1 - p otherwise, computed by the caller's libm once).  Same words consumed as numpy; the normals may differ from
 * numpy's in the last places (the device's log), the binomials are equal. */
int hp_rng_standard_normal(hp_rng *rng, int64_t count, double *host_out);
int hp_rng_binomial1(hp_rng *rng, double p, double qn, int64_t count, int64_t *host_out);
/* numpy's cached second normal (fields 3 and 4 of the legacy state tuple) lives next to (key, pos) on the device.  hp_rng_seed and
 * hp_rng_set_state clear it (np.random.seed does; a caller restoring a 5-tuple calls hp_rng_set_gauss after hp_rng_set_state).
 * Both synchronise. */
int hp_rng_get_gauss(hp_rng *rng, int32_t *has_gauss, double *gauss);
int hp_rng_set_gauss(hp_rng *rng, int32_t has_gauss, double gauss);
/* Skip n_words 32-bit words of the stream as if they had been drawn and thrown away (RandomState.bytes(4 * n_words)), without
 * walking to them: MT19937 is linear over GF(2), the key block at any offset is an XOR of windows of the next 19937 + 623 words
 * selected by x^J mod the generator's characteristic polynomial (jump-ahead; Haramoto et al. 2008).  hp_rng_get_state afterwards
 * equals numpy's (key, pos) bit for bit, word 0 and the pos = 624 boundary rule included.  n_words < 2^62.  Synchronises. */
int hp_rng_advance(hp_rng *rng, uint64_t n_words);
/* Parallel form of the sampler's index draw (her.py:24-33) -- the REFERENCE's stream, the same words in the same order, only not
 * walked by one workgroup: the stream is entered at every 16th block at once (jump-ahead), written out raw, and the four draws
 * of a batch (randint(N), randint(T), two uniforms) run over it as device-wide passes.  min_batch <= 0: off (the default; nothing
 * changes for anyone).  min_batch > 0: every index draw of hp_buffer_sample, hp_buffer_sample_dev and hp_buffer_sample_dev_f32 with
 * batch >= min_batch takes it; indices, outputs and the stream state afterwards are bit-identical to the sequential draw, which
 * stays enqueued behind it and does the work in the (probability < 2^-64) case that a batch consumes more words than were laid out.
 * HP_PARALLEL_DRAW_MIN_BATCH is the measured crossover.  Asynchronous and capturable like the calls it serves, except
 * that the first draw of a larger batch than any before allocates scratch: inside a stream capture such a draw stays sequential.
 * The fused learner's own plan draws (hp_agent_sample_and_update, hp_agent_train_cycle) never take this path. */
#define HP_PARALLEL_DRAW_MIN_BATCH 65536
int hp_rng_set_parallel(hp_rng *rng, int64_t min_batch);
void hp_rng_destroy(hp_rng *rng);

/* ---- episodic replay buffer ------------------------------------------------------------
 * replay_buffer.py:11-71.  Storage is float64 [size, T+1, obs], [size, T+1, goal],
 * [size, T, goal], [size, T, action] in HBM (same layout as the reference's numpy arrays). */
int hp_buffer_create(hp_ctx *ctx, int64_t size_episodes, int32_t T, int32_t obs_dim, int32_t goal_dim,
                     int32_t act_dim, hp_buffer **out);
/* replay_buffer.store_episode (:32-43) + _get_storage_idx (:57-71).  Host arrays, float64,
 * C-contiguous [n_new, T+1, obs] / [n_new, T+1, goal] / [n_new, T, goal] / [n_new, T, action].
 * Slot selection runs on the device and draws from `rng` exactly when the reference does. */
int hp_buffer_store(hp_buffer *buf, hp_rng *rng, const double *obs, const double *ag, const double *g,
                    const double *actions, int64_t n_new);
/* Upload n_new episodes into the buffer's device staging area WITHOUT storing them (no slot draw, counters untouched):
 * the temporary dict ddpg_agent._update_normalizer builds from the episodes it is handed (ddpg_agent.py:187-203).
 * hp_norm_update_from_staged then samples from exactly these episodes.  n_new == 0 -> "high <= 0" like numpy. */
int hp_buffer_stage(hp_buffer *buf, const double *obs, const double *ag, const double *g, const double *actions,
                    int64_t n_new);
/* Multi-process host feeder (the rollout workers of ddpg_agent.py:101-142 as processes): the episodes of a wave are
 * written by the workers into ONE host block [obs n x (T+1) x obs_dim | ag | g | actions] that the trainer registered
 * with the device (hp_host_register, e.g. a POSIX shared-memory segment).  hp_buffer_store_pinned is store_episode on
 * such a block without the CPU copy: the DMA reads the block directly and asynchronously (slot draw and scatter as in
 * hp_buffer_store); the block may be rewritten once hp_buffer_store_done reports its ticket done (wait != 0 blocks,
 * outside the context lock). */
int hp_host_register(hp_ctx *ctx, void *host, size_t bytes);
int hp_host_unregister(hp_ctx *ctx, void *host);
int hp_buffer_store_pinned(hp_buffer *buf, hp_rng *rng, const double *block, int64_t n_new, uint64_t *ticket);
int hp_buffer_store_done(hp_buffer *buf, uint64_t ticket, int32_t wait, int32_t *done);
/* store_episode on a block of the same layout that lies in DEVICE memory (a wave collected by hp_rollout_step): a device-to-device
 * copy in stream order, same slot draw and scatter; no ticket -- the block may be rewritten by later work on the stream. */
int hp_buffer_store_dev(hp_buffer *buf, hp_rng *rng, const double *block_dev, int64_t n_new);
int hp_buffer_info(hp_buffer *buf, int64_t *size, int64_t *current_size, int64_t *n_transitions_stored,
                   int32_t *T);
/* slots chosen by the most recent hp_buffer_store (parity tests); synchronises */
int hp_buffer_last_slots(hp_buffer *buf, int64_t *host_out, int64_t n);
/* copy episodes [first, first+n) of one array back to the host: which = 0 obs, 1 ag, 2 g, 3 actions */
int hp_buffer_read(hp_buffer *buf, int32_t which, int64_t first, int64_t n, double *host_out);

/* replay_buffer.sample (:46-55) -> her_sampler.sample_her_transitions (her.py:13-41) with the
 * sparse goal-distance reward of bmirobot_env_push_F.py:20-23,84-90 inlined.
 *   future_p      her.py:8  (1 - 1/(1+replay_k));  0 disables relabelling
 *   sq_threshold  smallest double s with sqrt(s) > distance_threshold (reward = -(s >= sq_threshold));
 *                 a NEGATIVE value selects the dense reward of compute_reward (:89-90): r = float32(-sqrt(s))
 * Any host output pointer may be NULL.  r is float32 [B] with bit patterns 0x80000000 / 0xBF800000.
 * e/t/future_t/her expose the drawn indices for parity tests (future_t is defined for every
 * sample; the reference uses it only where her != 0). */
typedef struct {
    double *obs, *ag, *g, *actions, *obs_next, *ag_next; /* [B, dim] float64 */
    float *r;                                            /* [B] */
    int64_t *e, *t, *future_t;                           /* [B] */
    uint8_t *her;                                        /* [B] */
    double *r64;                                         /* [B] what compute_reward itself returns: the float32 reward
                                                            widened (sparse) or -d in float64 (dense, :89-90) */
} hp_sample_out;
int hp_buffer_sample(hp_buffer *buf, hp_rng *rng, int64_t batch, double future_p, double sq_threshold,
                     const hp_sample_out *host_out);

/* replay_buffer.sample (:46-55) followed by the learner's own preprocessing of the minibatch (ddpg_agent.py:227-243:
 * _preproc_og clip :214-217, o_norm / g_norm .normalize normalizer.py:67-70, np.concatenate, torch.tensor(.., float32)) in ONE
 * gather kernel with DEVICE outputs -- the `hp_sample(... out device ptrs x, x', a, r)` of SURVEY.md section 8b.  What a
 * GPU learner consumes never crosses PCIe:
 *   x        float32 [B, obs+goal]  inputs_norm_tensor       (ddpg_agent.py:236,240)
 *   x_next   float32 [B, obs+goal]  inputs_next_norm_tensor  (:237,241)
 *   actions  float32 [B, act]       actions_tensor           (:242; unscaled, the critic divides by max_action itself)
 *   r        float32 [B]            r_tensor                 (:243; reshape to [B, 1])
 *   e, t, future_t (int64 [B]), her (uint8 [B]): the drawn indices, for parity tests
 * Any pointer may be NULL.  The normalizers' default_clip_range is the clip of normalize(); clip_obs is arguments.py:87.
 * Same random stream, same draws and same float64 arithmetic as hp_buffer_sample + hp_norm_normalize (bit-identical
 * float32 results).  Asynchronous on the context's stream; outputs are caller-owned device memory (torch tensors). */
typedef struct {
    float *x, *x_next, *actions, *r;
    int64_t *e, *t, *future_t;
    uint8_t *her;
} hp_sample_dev_out;
int hp_buffer_sample_dev(hp_buffer *buf, hp_rng *rng, hp_norm *o_norm, hp_norm *g_norm, int64_t batch, double future_p,
                         double sq_threshold, double clip_obs, const hp_sample_dev_out *dev_out);
/* Throughput mode of the sampler (SURVEY 8b's `storage_dtype` = fp32; opt-in, NOT bit-identical to the reference's float64 rows):
 * hp_buffer_enable_f32_rows builds -- from what the buffer holds now, and behind every later store, those of cycles whose graph was
 * captured before included (they are captured again) -- a float32 mirror of the observations and actions laid out for the gather
 * (one (episode, timestep) per 128-byte line: obs_t | action_t), the goals
 * staying float64.  hp_buffer_sample_dev_f32 = hp_buffer_sample_dev reading that mirror: same stream, same draws, indices,
 * relabelled goals (her.py:35-36), rewards (:38) and goal columns of x / x_next BIT-identical; actions identical (the learner takes
 * float32(actions) either way); the observation columns are those of float32-rounded observations (replay_buffer.py:23-27 stores
 * float64), about half the bytes per transition.  Needs obs_dim + act_dim <= 32.  The float64 arrays stay the source of truth:
 * hp_buffer_sample / hp_buffer_sample_dev / the fused learner are unaffected. */
int hp_buffer_enable_f32_rows(hp_buffer *buf);
int hp_buffer_sample_dev_f32(hp_buffer *buf, hp_rng *rng, hp_norm *o_norm, hp_norm *g_norm, int64_t batch, double future_p,
                             double sq_threshold, double clip_obs, const hp_sample_dev_out *dev_out);
/* Fast draw (SURVEY 8b's `rng_mode` = Philox; opt-in, NOT the reference's random stream): the same device-output minibatch with the
 * index draw inside the gather kernel -- no hp_rng, no sequential draw launch.  Transition m of call `call` takes
 * (r0..r3) = Philox4x32-10(counter (m, call), key `seed`) [Random123] and draws her.py:24-33's four values from them:
 * e = floor(r0 N / 2^32), t = floor(r1 T / 2^32), her = r2 2^-32 < future_p, future_t = t + 1 + floor(r3 (T - t) / 2^32).
 * Deterministic in (seed, call): the caller owns the counter (a rank passes seed + rank and call = 0, 1, 2, ...).  f32_rows != 0
 * reads the throughput rows.  Gather, relabel, reward, clip and normalisation are those of hp_buffer_sample_dev, bit for bit. */
int hp_buffer_sample_dev_fast(hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, int64_t batch, double future_p, double sq_threshold,
                              double clip_obs, uint64_t seed, uint64_t call, int32_t f32_rows, const hp_sample_dev_out *dev_out);

/* ---- GoalEnv reward / success as batched device ops --------------------------------------------
 * compute_reward (bmirobot_env_push_F.py:84-90 -> goal_distance :20-23; byte-identical in
 * bmirobot_env_pickandplace_v2.py:84-90) and _is_success (:243-245) for n goal pairs [n][goal_dim] float64.
 *   dense == 0: sparse reward -(d > distance_threshold).astype(float32) -> sparse_out (bits 0x80000000 / 0xBF800000)
 *   dense != 0: -d in float64 -> dense_out
 *   hp_is_success: (d < distance_threshold).astype(float32)
 * The predicates are evaluated on the squared distance against the smallest double whose correctly rounded square
 * root passes the comparison, so they agree with numpy's sqrt-then-compare for every input (bit-exact for
 * goal_dim < 8, where numpy's add.reduce is a left-to-right sum).  *_dev: device pointers, asynchronous on the context's
 * stream; the plain forms take host arrays and synchronise. */
int hp_compute_reward_dev(hp_ctx *ctx, const double *ag_dev, const double *g_dev, int64_t n, int32_t goal_dim,
                          double distance_threshold, int32_t dense, float *sparse_out_dev, double *dense_out_dev);
int hp_is_success_dev(hp_ctx *ctx, const double *ag_dev, const double *g_dev, int64_t n, int32_t goal_dim,
                      double distance_threshold, float *out_dev);
int hp_compute_reward(hp_ctx *ctx, const double *ag_host, const double *g_host, int64_t n, int32_t goal_dim,
                      double distance_threshold, int32_t dense, float *sparse_out_host, double *dense_out_host);
int hp_is_success(hp_ctx *ctx, const double *ag_host, const double *g_host, int64_t n, int32_t goal_dim,
                  double distance_threshold, float *out_host);

/* ---- running normalizer ----------------------------------------------------------------
 * normalizer.py:5-70.  float32 accumulators/totals/mean; std is float64 when std_f32 == 0
 * (what numpy >= 2 computes for the reference's expression) or float32 when std_f32 != 0
 * (numpy 1.19.2, the version the reference pins). */
int hp_norm_create(hp_ctx *ctx, int32_t size, double eps, double default_clip_range, int32_t std_f32,
                   hp_norm **out);
int hp_norm_update(hp_norm *nz, const double *v_host, int64_t rows);          /* normalizer.update :25-31 */
/* normalizer.recompute_stats :40-57 split around the cross-rank mean (:34-38, :60-64):
 *   begin: snapshot + zero the local accumulators; *dev_sync -> float32[2*size+1] = sum|sumsq|count
 *   (caller all-reduces that vector and divides by world size -- RCCL -- or leaves it alone)
 *   end:   totals += sync; mean/std recomputed. */
int hp_norm_recompute_begin(hp_norm *nz, void **dev_sync, int64_t *n_floats);
int hp_norm_recompute_end(hp_norm *nz);
int hp_norm_recompute(hp_norm *nz);                                            /* single-rank: begin+end */
/* host copies of the state (any pointer may be NULL); synchronises */
int hp_norm_get(hp_norm *nz, float *mean, double *std, float *total_sum, float *total_sumsq, float *total_count,
                float *local_sum, float *local_sumsq, float *local_count);
int hp_norm_set_stats(hp_norm *nz, const float *mean, const double *std);    /* checkpoint load */
/* normalizer.normalize :67-70 on host data (rollout / test path).  clip_range < 0 -> default */
int hp_norm_normalize(hp_norm *nz, const double *v_host, int64_t rows, double clip_range, double *out_host);

/* ddpg_agent._update_normalizer (:187-212): HER-sample T transitions out of the n_new
 * episodes most recently passed to hp_buffer_store (still staged on the device), clip to
 * +-clip_obs (:214-217), update both normalizers.  Does NOT recompute (call hp_norm_recompute*). */
int hp_norm_update_from_staged(hp_buffer *buf, hp_rng *rng, hp_norm *o_norm, hp_norm *g_norm, double future_p,
                               double clip_obs);

/* ---- DDPG learner -----------------------------------------------------------------------
 * models.py:11-44 (actor 30-256-256-256-4, critic 34-256-256-256-1), ddpg_agent.py:220-277,
 * torch.optim.Adam defaults (ddpg_agent.py:42-43), utils.py:6-69 flat parameter order. */
typedef struct {
    int32_t obs_dim, goal_dim, act_dim, hidden;
    int32_t batch;           /* transitions per update (arguments.py:88) */
    int32_t grad_world_size; /* informational (grads are SUMmed across ranks, utils.py:47) */
    /* Python floats in the reference -> doubles here; they are narrowed to float32 exactly where
     * torch narrows them (tensor-scalar ops) so the arithmetic matches. */
    double max_action;       /* env action_max (bmirobot_env_push_F.py:75-78) */
    double gamma;            /* arguments.py:89 */
    double action_l2;        /* arguments.py:90 */
    double lr_actor, lr_critic; /* arguments.py:91-92 */
    double polyak;           /* arguments.py:93 */
    double clip_obs;         /* arguments.py:87 */
    double clip_range;       /* arguments.py:95 (normalizer default_clip_range) */
    double adam_beta1, adam_beta2, adam_eps; /* torch.optim.Adam defaults 0.9, 0.999, 1e-8 */
} hp_agent_cfg;

enum { HP_NET_ACTOR = 0, HP_NET_CRITIC = 1, HP_NET_ACTOR_TARGET = 2, HP_NET_CRITIC_TARGET = 3 };

int hp_agent_create(hp_ctx *ctx, const hp_agent_cfg *cfg, hp_agent **out);
int64_t hp_agent_param_count(hp_agent *ag, int32_t net);   /* 140548 / 140801 for the reference sizes */
/* flat float32 vectors in named_parameters() order (utils.py:18-40): fc1.weight, fc1.bias, ... */
int hp_agent_set_params(hp_agent *ag, int32_t net, const float *flat_host, int64_t n);
int hp_agent_get_params(hp_agent *ag, int32_t net, float *flat_host, int64_t n);
/* gradients of the last hp_agent_update_minibatch / hp_agent_forward_backward (the sampled update loops of a single
 * rank consume the weight gradients in the optimizer epilogue without writing them out; bias gradients are always
 * written) */
int hp_agent_get_grads(hp_agent *ag, int32_t net, float *flat_host, int64_t n);  /* net = actor|critic */
int hp_agent_get_adam(hp_agent *ag, int32_t net, float *m_host, float *v_host, int64_t n, int64_t *step);

/* One ddpg_agent._update_network (:250-277) on a caller-provided, already normalised minibatch
 * (host float32: x [B,obs+goal], x_next [B,obs+goal], actions [B,act], r [B]).
 * losses_host[0] = actor_loss, [1] = critic_loss.  Synchronises. */
int hp_agent_update_minibatch(hp_agent *ag, const float *x, const float *x_next, const float *actions,
                              const float *r, float *losses_host);

/* The hot loop (ddpg_agent.py:145-147): n_updates x { sample B transitions, relabel, reward, clip,
 * normalise, 5 forwards, 3 backwards, Adam x2 } entirely on the device.  Asynchronous. */
int hp_agent_sample_and_update(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng,
                               double future_p, double sq_threshold, int32_t n_updates);
/* losses of the most recent updates, newest last: out[2*i] actor, out[2*i+1] critic.  Synchronises. */
int hp_agent_get_losses(hp_agent *ag, float *out_host, int32_t n_last);
/* ddpg_agent._soft_update_target_network (:220-222) for both nets.  Asynchronous. */
int hp_agent_soft_update(hp_agent *ag);
/* actor forward on host inputs (rollout side, ddpg_agent.py:114-116): x [rows, obs+goal] -> actions [rows, act] */
int hp_agent_actor_forward(hp_agent *ag, int32_t net, const float *x_host, int64_t rows, float *actions_host);
/* critic forward on host inputs (models.py:28-44: the critic scales the actions by 1/max_action itself):
 * x [rows, obs+goal] float32 (normalised), actions [rows, act] float32 -> q [rows] */
int hp_agent_critic_forward(hp_agent *ag, int32_t net, const float *x_host, const float *actions_host, int64_t rows,
                            float *q_host);
/* rollout side in one call (ddpg_agent._preproc_inputs :163-171 + actor, :114-116 / :288-292): float64 observation
 * and goal rows -> normalise with the two normalizers (clip at each normalizer's default_clip_range), float32, actor
 * forward -> actions [rows, act].  clip_obs > 0 additionally clips the raw values first (_preproc_og); the reference's
 * rollouts do not, so the drop-in passes 0.  rows = the environments of a vectorised feeder stepped in lockstep. */
int hp_agent_act(hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t net, const double *obs_host,
                 const double *g_host, int64_t rows, double clip_obs, float *actions_host);
/* The same call on rows that lie in device memory (a vectorised simulator's tensors): same kernels, same bits, actions written to
 * device memory; asynchronous on the context's stream, nothing is copied and nothing waits. */
int hp_agent_act_dev(hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t net, const double *obs_dev,
                     const double *g_dev, int64_t rows, double clip_obs, float *actions_dev);

/* ---- rollouts collected on the device (ddpg_agent.py:101-137 for a vectorised simulator in device memory) -----------------
 * A wave block holds n_envs episodes in the layout of hp_buffer_store_pinned (dims and T from `buf`).  Per timestep
 * hp_rollout_step records the current rows (obs[i,t], ag[i,t], g[i,t]), evaluates the online actor as hp_agent_act_dev does
 * (clip_obs = 0) into actions_f32_dev, and -- explore != 0 -- applies ddpg_agent._select_actions (:174-184) to every row in
 * the host's order (env i = 0 .. n-1: randn(act), uniform(act), binomial(1, random_eps)) out of `rng`'s stream; qn as
 * hp_rng_binomial1.  clip_abs > 0 clips the action to +-clip_abs (:118-119).  actions[i,t] is recorded as float64, the float32
 * actions stay in actions_f32_dev for the simulator.  ag == NULL: actions_f32_dev already holds the policy outputs (action_max
 * from hp_rollout_set_action_max).  Two launches per timestep, asynchronous, no host copy.  hp_rollout_finish records row T.
 * hp_rollout_begin selects the episodes [first, first + n_rows) of the block as the wave the following calls step (default: all
 * n_envs), so more episodes than simulator instances are collected wave after wave into one block.  hp_rollout_read copies one
 * array (0 obs, 1 ag, 2 g, 3 actions) to the host and synchronises. */
int hp_rollout_create(hp_ctx *ctx, hp_buffer *buf, int64_t n_envs, hp_rollout **out);
int hp_rollout_begin(hp_rollout *ro, int64_t first_episode, int64_t n_rows);
int hp_rollout_set_action_max(hp_rollout *ro, double action_max);
int hp_rollout_step(hp_rollout *ro, hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng, int32_t t,
                    const double *obs_dev, const double *ag_dev, const double *g_dev, int32_t explore, double noise_eps,
                    double random_eps, double qn, double clip_abs, float *actions_f32_dev);
int hp_rollout_finish(hp_rollout *ro, const double *obs_dev, const double *ag_dev);
int hp_rollout_block(hp_rollout *ro, void **block_dev, int64_t *n_episodes, int64_t *offsets4, int64_t *elems);
int hp_rollout_read(hp_rollout *ro, int32_t which, double *host_out);
void hp_rollout_destroy(hp_rollout *ro);

/* ---- one exploration stream per environment ---------------------------------------------------------------------------------
 * The reference gives every MPI rank one environment and one numpy stream seeded `seed + rank` (train.py:34-39) and lets the rank
 * drive _select_actions (ddpg_agent.py:174-184) alone.  An hp_rng_streams is n such streams side by side in device memory: stream i
 * is a whole legacy state (key[624], pos, has_gauss, cached normal) interoperable with np.random.RandomState(seed_i).get_state().
 * hp_streams_create seeds every stream with numpy's default key (5489); hp_streams_seed seeds stream i with seeds_host[i]
 * (n_seeds must be the stream count) or, seeds_host == NULL, with base_seed + i -- n init_genrand recurrences run on the device,
 * one per stream -- and clears the cached normals.  get / set of one state and of all states (keys [n][624], pos / has_gauss /
 * gauss [n]) synchronise.
 * hp_rollout_step_streams is hp_rollout_step with the stream array in place of the single stream: row i of the wave draws
 * randn(act), uniform(act), binomial(1, random_eps) out of stream i alone, so what an environment draws depends neither on the
 * number of environments nor on the wave it is part of, and a wave of k rows (hp_rollout_begin) advances streams 0 .. k-1 only.
 * Rounding points, qn, clip_abs and the teacher-forced form (ag == NULL) are hp_rollout_step's; the draw launch has one wave per
 * row instead of one wave for all rows.  explore == 0 touches no stream (streams may be NULL).  A wave wider than the array is
 * refused. */
int hp_streams_create(hp_ctx *ctx, int64_t n, hp_rng_streams **out);
int hp_streams_seed(hp_rng_streams *s, const uint32_t *seeds_host, int64_t n_seeds, uint32_t base_seed);
int hp_streams_get_state(hp_rng_streams *s, int64_t i, uint32_t *key624, int32_t *pos, int32_t *has_gauss, double *gauss);
int hp_streams_set_state(hp_rng_streams *s, int64_t i, const uint32_t *key624, int32_t pos, int32_t has_gauss, double gauss);
int hp_streams_get_all(hp_rng_streams *s, uint32_t *keys, int32_t *pos, int32_t *has_gauss, double *gauss);
int hp_streams_set_all(hp_rng_streams *s, const uint32_t *keys, const int32_t *pos, const int32_t *has_gauss, const double *gauss);
void hp_streams_destroy(hp_rng_streams *s);
int hp_rollout_step_streams(hp_rollout *ro, hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, hp_rng_streams *streams, int32_t t,
                            const double *obs_dev, const double *ag_dev, const double *g_dev, int32_t explore, double noise_eps,
                            double random_eps, double qn, double clip_abs, float *actions_f32_dev);

/* ---- whole episodes in one launch, for environments the library steps itself -------------------------------------------------
 * For an environment whose dynamics the library can evaluate (an analytic, vectorised simulator) the T timesteps of a wave need
 * no launch boundary: hp_rollout_episodes collects the wave selected by hp_rollout_begin -- `rows` episodes, row i on stream i --
 * in ONE launch.  Workgroup b owns rows 4b .. 4b+3 and loops over t: observe, record obs / ag / g [i,t], the policy of
 * hp_agent_act_dev (clip_obs = 0), exploration as hp_rollout_step_streams (explore != 0) or the noise-free branch of
 * hp_rollout_step (explore == 0: streams may be NULL, no stream is touched), record actions[i,t], step.  Then row T is recorded,
 * success_dev[i] (float32 [rows]) receives is_success of the last step and the environment's final state is written back.  Block,
 * stream states and environment state are bit for bit what T per-step launches around the same arithmetic in torch leave.
 * Asynchronous on the context's stream, capturable.  Needs the agent the fused policy kernel serves (hidden 256, padded input
 * width <= 48, at most 4 action components: hp_agent_engine reports 8); any other agent is refused and keeps the per-step calls.
 * HP_ERR_INVALID names the field for: an unknown kind, dimensions of block / agent / normalizers / environment that differ, a
 * wave wider than the stream array, explore != 0 without streams, an agent of another shape.
 * Adding an environment kind is a build-time change: one struct in csrc/env_device.h (load, observe, step, is_success, store
 * over the arrays of hp_env_desc, with its dimensions as constants), its row in the table of kinds of csrc/rollout.hip, and
 * translation units that instantiate the kernel templates (csrc/rollout_episodes.h, csrc/demo_episodes.h) for that struct; the
 * header of csrc/env_device.h has the whole list.
 * HP_ENV_PUSH_BLOCK is a kinematic planar push: the achieved goal is a block that moves only while the gripper touches it, and
 * its reset redraws block and target until they are min_separation apart (at most 100 attempts: csrc/env_device.h).
 * HP_ENV_PICK_PLACE is a kinematic pick-and-place: the goal hangs in the air, the block is a cube that moves only in a closed
 * hand -- grasped when open fingers close with the finger pads inside it, and never released (the environment keeps a held
 * block's fingers closing, the reference's finger lock) -- the fourth action component moves the fingers, and the reset is the
 * push block's rejection loop in three dimensions, five draws an attempt. */
enum { HP_ENV_POINT_MASS = 1 };
enum { HP_ENV_PUSH_BLOCK = 2 };
enum { HP_ENV_PICK_PLACE = 3 };
typedef struct {
    int32_t kind, reserved;
    double params[8];         /* point mass: [0] step_scale, [1] distance_threshold
                               * push block: [0] step_scale, [1] distance_threshold, [2] half_width, [3] z_touch, [4] min_separation,
                               *             [5] table_z, [6] [7] gripper start x, y
                               * pick and place: [0] step_scale, [1] distance_threshold, [2] half_width, [3] finger_scale,
                               *             [4] min_separation, [5] table_z, [6] [7] gripper start x, y */
    double *state_dev[4];     /* read at entry, written at exit; a kind's unused slots are ignored
                               * point mass: [0] pos [n][3], [1] vel [n][3], [2] goal [n][3]
                               * push block: [0] gripper [n][3], [1] block [n][3], [2] goal [n][3], [3] velocities [n][6] (gripper, block)
                               * pick and place: [0] gripper [n][3], [1] block [n][3], [2] goal [n][3], [3] [n][8] = gripper velocity,
                               *             block velocity, finger opening, held (0.0 or 1.0) */
} hp_env_desc;
int hp_rollout_episodes(hp_rollout *ro, hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, hp_rng_streams *streams,
                        const hp_env_desc *env, int32_t explore, double noise_eps, double random_eps, double qn,
                        double clip_abs, float *success_dev);

/* ---- environments reset on the device; all waves of a call in one launch ------------------------------------------------------
 * An environment kind may declare a reset (csrc/env_device.h): a fixed number of random_uniform(low, range) draws -- or, for a
 * kind whose host reset is a rejection loop (push block), that many draws per attempt, repeated until the attempt is accepted
 * or the kind's attempts are spent -- out of the environment's own reset stream -- stream i of an hp_rng_streams, np.random.RandomState's legacy state like the exploration
 * streams -- and the fresh state built from them.  Point mass: six draws of uniform(0, 0.5), pos = u[0:3], goal = u[3:6], vel = 0,
 * the twelve words of the host twin's two uniform(0, 0.5, 3) calls.
 * hp_env_reset resets environments 0 .. rows-1 of the arrays of `env` (one wave per environment: load stream i, draw, write the
 * state, commit the stream in numpy's lazy form); environments and streams >= rows are untouched.  Asynchronous on the context's
 * stream (or a borrowed one).
 * hp_rollout_waves is hp_rollout_episodes for a call of more episodes than environments: the `rows` episodes selected by
 * hp_rollout_begin (rows may exceed n_envs) are collected as ceil(rows / n_envs) waves inside ONE launch.  The state arrays of
 * `env` hold n_envs environments.  Workgroup b owns environments 4b .. 4b+3 and loops over the waves: environment i takes part in
 * wave w if w * n_envs + i < rows, is then reset from reset stream i, runs T timesteps as in hp_rollout_episodes and is recorded
 * as episode first + w * n_envs + i; success_dev[w * n_envs + i] receives its flag.  Exploration stream i runs on across the waves
 * of a launch; a partial last wave touches neither stream of the environments it leaves out.  At the end every environment's
 * state, goal included, and every stream are written back once.  The bits are those of ceil(rows / n_envs) calls of hp_env_reset
 * + hp_rollout_episodes.  A launch holds at most HP_ROLLOUT_MAX_LAUNCH_TIMESTEPS timesteps (whole waves of T, at least one):
 * longer calls are issued as consecutive launches, and *launches_out (may be NULL) receives how many there were.  4096: at the
 * measured 9.3 us (up to 64 environments) to 31 us (1024 environments) per timestep of the fused kernel a launch ends after 40 to
 * 130 ms, well under a second on a device other work shares.
 * HP_ERR_INVALID, naming the entry point, for: a null argument, handles of different contexts, fewer reset streams than n_envs
 * (hp_env_reset: than rows), episodes outside the block, a kind without a reset, and everything hp_rollout_episodes refuses. */
#define HP_ROLLOUT_MAX_LAUNCH_TIMESTEPS 4096
int hp_env_reset(hp_ctx *ctx, const hp_env_desc *env, hp_rng_streams *reset_streams, int64_t rows);
int hp_rollout_waves(hp_rollout *ro, hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, hp_rng_streams *streams,
                     hp_rng_streams *reset_streams, const hp_env_desc *env, int64_t n_envs, int32_t explore, double noise_eps,
                     double random_eps, double qn, double clip_abs, float *success_dev, int32_t *launches_out);

/* ---- demonstration episodes from a scripted controller, generated on the device ---------------------------------------------
 * The reference fills its replay buffer with episodes a scripted push controller produced (get_demo_data_push.py:24-94) and
 * keeps the successful ones.  hp_demo_script holds that controller's numbers (defaults: the reference's, in
 * synthetic.DemoScript): timestep t = 1 .. T is in phase p if it is <= phase_end[p] and in no earlier phase, in the sixth phase
 * behind phase_end[4].  Phase one: the constant action `lift`; two and five: go behind the block,
 * ((g - b) * behind + b) - grip; three and six: push, g - b; four: to the waypoint, waypoint - grip (fourth component 0 from
 * phase two on), with grip = obs[0:3], b = obs[12:15], g the desired goal; and the action is all zeros once
 * sqrt(dx dx + dy dy + dz dz) < stop_radius between b and g.  Every float64 operation is rounded on its own, sums left to right.
 * hp_demo_episodes collects `n_episodes` scripted episodes of a native environment kind with a reset on the device into episodes
 * [first_episode, first_episode + n_episodes) of `block` (the block of an hp_rollout: T and the dimensions are its own), as
 * ceil(n_episodes / n_envs) waves: workgroup i is one wave and owns environment i and reset stream i; episode w * n_envs + i is
 * environment i's w-th -- reset from its stream, then T timesteps of observe, controller, record, step -- and an environment
 * whose episode number falls behind n_episodes touches neither its stream nor its state.  The controller's float64 action is
 * recorded as it is; the environment clips what it applies.  success_dev [n_episodes] and step_success_dev [n_episodes][T]
 * (float32) receive is_success after the last and after every step.  No agent, no weights.  Streams and environment states are
 * written back once per launch; a launch holds at most HP_ROLLOUT_MAX_LAUNCH_TIMESTEPS timesteps as in hp_rollout_waves (the
 * block's own cap), *launches_out (may be NULL) says how many there were.
 * hp_demo_compact is the success filter, order preserving: episode e of the first n_episodes of `src` with success_dev[e] != 0
 * and rank r among those is copied -- obs, ag, g, actions and its row of step_success_dev -- to episode kept + r of `dst` (and
 * row kept + r of dst_step_success_dev) if that is < n_demos; *kept_dev (int32, device) receives min(kept + successes, n_demos).
 * `kept` is what the caller read after the previous round (0 at first).
 * Both asynchronous on the context's stream (or a borrowed one).  HP_ERR_INVALID, naming the entry point, for: a null argument,
 * handles of different contexts, an unknown kind or one without a reset on the device, a null state array, n_envs wider than
 * the stream array, T or dimensions that differ from the block's (hp_demo_compact: between the blocks), episodes outside a
 * block, phase ends that are not increasing.
 * hp_demo_episodes_pick is hp_demo_episodes with the reference's pick-and-place schedule (get_demo_data_pick.py:54-67,
 * synthetic.pick_scripted_action) in place of the push schedule, and hp_pick_script holds its numbers (defaults in
 * synthetic.PickScript): phases as above; one: the constant action `lift`; two: (b - grip) + approach; three: the fingers,
 * (0, 0, 0, open); four: (b - grip) + grasp; five: (0, 0, 0, -open); six: g - b (fourth component 0 in two, four and six).  No
 * stop rule.  Everything else -- arguments, waves, launches, refusals (naming hp_demo_episodes_pick) -- is hp_demo_episodes'.
 * A controller is no property of an environment kind: either entry runs on any kind with a reset on the device. */
typedef struct {
    int32_t phase_end[5];     /* last timestep (counted from 1) of phases one to five */
    int32_t reserved;
    double lift[4];           /* the action of phase one */
    double waypoint[3];       /* where phase four takes the gripper */
    double behind;            /* -0.5: how far behind the block, in units of the block-to-goal vector */
    double stop_radius;       /* 0.05 */
} hp_demo_script;
int hp_demo_episodes(hp_ctx *ctx, const hp_env_desc *env, hp_rng_streams *reset_streams, const hp_demo_script *script,
                     int64_t n_envs, int64_t first_episode, int64_t n_episodes, int32_t T, hp_rollout *block, float *success_dev,
                     float *step_success_dev, int32_t *launches_out);
typedef struct {
    int32_t phase_end[5], reserved;   /* last timestep (counted from 1) of phases one to five */
    double lift[4], approach[3], grasp[3], open;   /* the action of phase one; the offsets of phases two and four; the finger action */
} hp_pick_script;
int hp_demo_episodes_pick(hp_ctx *ctx, const hp_env_desc *env, hp_rng_streams *reset_streams, const hp_pick_script *script,
                          int64_t n_envs, int64_t first_episode, int64_t n_episodes, int32_t T, hp_rollout *block, float *success_dev,
                          float *step_success_dev, int32_t *launches_out);
int hp_demo_compact(hp_ctx *ctx, hp_rollout *src, const float *success_dev, const float *step_success_dev, int64_t n_episodes,
                    hp_rollout *dst, float *dst_step_success_dev, int64_t n_demos, int64_t kept, int32_t *kept_dev);

/* ---- episode metrics on the device ------------------------------------------------------------
 * The reference records info['is_success'] at every step of every evaluation episode and keeps the last (ddpg_agent.py:280-304);
 * these entries keep the rest, computed where the episodes lie.  ag_dev is [n_episodes][T + 1][goal_dim] and g_dev
 * [n_episodes][T][goal_dim], float64 and contiguous: the layout of a block's own arrays (hp_rollout_block).  Step t = 0 .. T-1
 * compares ag[t + 1] with g[t] (her.py:38, _is_success); d[t] = sqrt(((dx dx + dy dy) + dz dz) ...), every product, sum and the
 * root rounded on its own, summed left to right over goal_dim -- np.linalg.norm(a - b, axis=-1) for goal_dim < 8; is_success is
 * hp_is_success_dev's rule and the reward hp_compute_reward_dev's sparse one.  stats_dev [n_episodes][HP_EPISODE_STATS], float64:
 *   [0] ret                 sum over t of the sparse reward, started at +0.0 (an episode that succeeds throughout: +0.0)
 *   [1] final_distance      d[T-1]
 *   [2] min_distance        min over t of d[t]
 *   [3] first_success_step  the smallest t with is_success, T if there is none
 *   [4] success_steps       the number of steps with is_success
 *   [5] final_success       0.0 or 1.0: is_success of step T-1, what success_dev of hp_rollout_episodes / hp_rollout_waves holds
 * step_success_dev [n_episodes][T] (float32, may be NULL) receives the flag of every step: the reference's per_success_rate, the
 * step_success_dev of hp_demo_episodes.  One wave per episode; every reduction (a sum of exact small integers, two minima, a
 * count) is order independent, so the bits are those of the host twin (synthetic.episode_stats) whatever the mapping.  Inputs
 * must be finite.  hp_episode_stats_block is the same on episodes [first_episode, first_episode + n_episodes) of a block, with T,
 * goal_dim and the arrays taken from the handle.
 * hp_episode_stats_summary reduces n_episodes rows of stats to summary_dev [HP_EPISODE_SUMMARY] (float64): the means of ret,
 * final_distance, min_distance and first_success_step, the success rate (mean of [5]) and the share of episodes with
 * success_steps > 0 -- each a left-to-right sum in episode order divided by n_episodes (one lane walks the rows: the order is
 * fixed, synthetic.episode_stats_summary is the same loop), so an evaluation reads 48 bytes once.
 * All three asynchronous on the context's stream (or a borrowed one); nothing is allocated.  HP_ERR_INVALID, naming the entry
 * point, for: a null argument (step_success_dev excepted), n_episodes < 1 (or 2^24 and more), T < 1, goal_dim outside
 * [1, HP_EPISODE_MAX_GOAL_DIM], episodes outside the block. */
#define HP_EPISODE_STATS 6
#define HP_EPISODE_SUMMARY 6
#define HP_EPISODE_MAX_GOAL_DIM 256   /* what a normalizer holds */
int hp_episode_stats(hp_ctx *ctx, const double *ag_dev, const double *g_dev, int64_t n_episodes, int32_t T, int32_t goal_dim,
                     double distance_threshold, double *stats_dev, float *step_success_dev);
int hp_episode_stats_block(hp_rollout *ro, int64_t first_episode, int64_t n_episodes, double distance_threshold, double *stats_dev,
                           float *step_success_dev);
int hp_episode_stats_summary(hp_ctx *ctx, const double *stats_dev, int64_t n_episodes, double *summary_dev);

/* ---- critic audit on the device ----------------------------------------------------------------
 * What the critic believes of an episode block beside what the episodes went on to collect: whether Q(s_t, a_t) tracks the
 * discounted return, sits on the target clip -1 / (1 - gamma) (ddpg_agent.py:259-260) or overestimates.
 *
 * hp_episode_q: q_dev[e][t] (float32) = critic(normalise(obs[e][t] | g[e][t]), actions[e][t] / max_action) for t = 0 .. T-1 of
 * n_episodes episodes in ONE launch.  obs_dev is [n_episodes][T + 1][obs_dim], g_dev [n_episodes][T][goal_dim], actions_dev
 * [n_episodes][T][act_dim], float64 and contiguous: a block's own arrays.  net is HP_NET_CRITIC or HP_NET_CRITIC_TARGET.  A row
 * enters the critic exactly as a transition enters an update: clip to +-clip_obs (<= 0: no clip), subtract the mean, divide by
 * the std, clip to the normalizer's range, each in float64 and rounded once, then float32; the action narrowed to float32 and
 * divided by max_action in float32.  The forward is the training chain's critic forward (same device functions, 4-row slabs), on
 * the weights every update launch form leaves behind, in stream order.  hp_episode_q_block is the same on episodes
 * [first_episode, first_episode + n_episodes) of a block.  Both asynchronous on the context's stream (or a borrowed one); nothing
 * is allocated.  Refused before anything is launched, naming the entry point: a null argument, handles of different contexts, a
 * net that is not a critic, episodes outside the block, normalizer or block dimensions that differ from the agent's (all
 * HP_ERR_INVALID), an agent that is not slab-shaped (HP_ERR_STATE, like hp_agent_policy_snapshot), n_episodes or T outside
 * [1, 2^24], more than 2^31 steps.
 *
 * hp_episode_returns: returns_dev[e][t] (float64) = G_t with G_t = r_t + gamma G_{t+1}, every operation rounded on its own;
 * r_t is compute_reward's on (ag[t + 1], g[t]) in float64 -- reward_type 0: sparse, -(d > distance_threshold), 1: dense, -d --
 * with the squared distance formed as hp_episode_stats forms it.  tail 0: G_T = +0.0; tail 1: G_T = r_{T-1} / (1 - gamma), the
 * last step's reward held for ever.  gamma must lie in [0, 1], and gamma = 1 with tail 1 is refused.  With q_dev [n][T]
 * (float32, hp_episode_q's output) and critic_stats_dev [n][HP_CRITIC_STATS] (float64; both or neither) every episode also gets
 *   [0] q_mean          mean over t of Q            [3] abs_error       mean of |Q - G|
 *   [1] return_mean     mean of G                   [4] max_abs_error   max of |Q - G|
 *   [2] bias            mean of Q - G               [5] floor_steps     steps with Q <= -1 / (1 - gamma) (0 when gamma = 1)
 * each sum accumulated in float64 in the order of the recursion, t = T-1 down to 0, and divided by T: the order is fixed, and
 * synthetic.episode_returns / episode_critic_stats are the same loops, so the bits are the host twin's.  One wave per episode.
 * hp_episode_returns_block is the same on a block's episodes.  hp_episode_critic_summary reduces n_episodes rows to the six
 * column means, left to right in episode order (synthetic.episode_critic_summary).  All asynchronous, nothing allocated;
 * HP_ERR_INVALID, naming the entry point, for a null argument (q_dev / critic_stats_dev excepted), n_episodes, T or goal_dim out
 * of range as for hp_episode_stats, an unknown reward_type or tail, gamma outside [0, 1], episodes outside the block. */
#define HP_CRITIC_STATS 6
int hp_episode_q(hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t net, const double *obs_dev, const double *g_dev,
                 const double *actions_dev, int64_t n_episodes, int32_t T, double clip_obs, float *q_dev);
int hp_episode_q_block(hp_rollout *ro, hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t net, int64_t first_episode,
                       int64_t n_episodes, double clip_obs, float *q_dev);
int hp_episode_returns(hp_ctx *ctx, const double *ag_dev, const double *g_dev, int64_t n_episodes, int32_t T, int32_t goal_dim,
                       double distance_threshold, int32_t reward_type, double gamma, int32_t tail, double *returns_dev,
                       const float *q_dev, double *critic_stats_dev);
int hp_episode_returns_block(hp_rollout *ro, int64_t first_episode, int64_t n_episodes, double distance_threshold,
                             int32_t reward_type, double gamma, int32_t tail, double *returns_dev, const float *q_dev,
                             double *critic_stats_dev);
int hp_episode_critic_summary(hp_ctx *ctx, const double *critic_stats_dev, int64_t n_episodes, double *summary_dev);

/* ---- policy audit on the device ----------------------------------------------------------------
 * What the actor's objective sees of an episode block: pi(s_t) and Q(s_t, pi(s_t)) beside the recorded action and hp_episode_q's
 * Q(s_t, a_t) -- whether the critic ranks a demonstration's action above the policy's (the Q-filter), how far the recorded
 * actions lie from the policy, whether the actor saturates its tanh; the two terms of the actor loss (ddpg_agent.py:265-267).
 *
 * hp_episode_policy: pi_dev[e][t][j] (float32) = max_action * tanh(actor(normalise(obs[e][t] | g[e][t]))) and q_pi_dev[e][t]
 * (float32) = critic(the same input, (max_action * tanh) / max_action) for t = 0 .. T-1 of n_episodes episodes in ONE launch:
 * the forward half of an update's actor-side chain (same device functions, 4-row slabs, the action input formed in float32
 * exactly as there) on rows that enter it as hp_episode_q's do.  obs_dev is [n_episodes][T + 1][obs_dim], g_dev
 * [n_episodes][T][goal_dim], float64 and contiguous.  target 0: online actor and critic; 1: target actor and target critic.
 * hp_episode_policy_block is the same on episodes [first_episode, first_episode + n_episodes) of a block.  Both asynchronous on
 * the context's stream (or a borrowed one), behind whatever wrote the weights; nothing is allocated.  Refusals are
 * hp_episode_q's, naming the entry point (target outside {0, 1} takes the place of the net).
 *
 * hp_episode_policy_stats: stats_dev [n][HP_POLICY_STATS] (float64) out of pi_dev, q_pi_dev, the recorded actions_dev
 * [n][T][act_dim] (float64) and q_dev [n][T] (float32, hp_episode_q's output on the same episodes; may be NULL: [1] and [2] are
 * then NaN).  With M = (double)(float)max_action:
 *   [0] q_pi_mean        sum_t Q(s_t, pi(s_t)) / T
 *   [1] advantage_mean   sum_t (Q(s_t, pi(s_t)) - Q(s_t, a_t)) / T
 *   [2] q_filter_share   #{t : Q(s_t, a_t) > Q(s_t, pi(s_t))} / T (float32 compare)
 *   [3] action_gap_mean  (sum_t sqrt(sum_j d_j d_j)) / M / T, d_j = a[t][j] - pi[t][j]
 *   [4] saturated_share  #{(t, j) : |pi[t][j]| >= sat * M} / (T act_dim), sat in [0, 1]
 *   [5] action_l2_mean   sum_t (sum_j v_j v_j / act_dim) / T, v_j = pi[t][j] / M
 * every float32 widened to float64, every sum started at 0 and accumulated in ascending t (inner j ascending), every operation
 * rounded on its own: the order is fixed and synthetic.episode_policy_stats is the same loop, so the bits are the host twin's.  One
 * wave per episode.  hp_episode_policy_stats_block takes the actions of a block's episodes.  hp_episode_policy_summary reduces
 * n_episodes rows to the six column means, left to right in episode order (synthetic.episode_policy_summary).  All asynchronous,
 * nothing allocated; HP_ERR_INVALID, naming the entry point, for a null argument (q_dev excepted), n_episodes or T out of range
 * as for hp_episode_stats, act_dim outside [1, HP_POLICY_MAX_ACT_DIM], max_action not positive and finite, sat outside [0, 1],
 * episodes outside the block. */
#define HP_POLICY_STATS 6
#define HP_POLICY_MAX_ACT_DIM 256
int hp_episode_policy(hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t target, const double *obs_dev, const double *g_dev,
                      int64_t n_episodes, int32_t T, double clip_obs, float *pi_dev, float *q_pi_dev);
int hp_episode_policy_block(hp_rollout *ro, hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t target, int64_t first_episode,
                            int64_t n_episodes, double clip_obs, float *pi_dev, float *q_pi_dev);
int hp_episode_policy_stats(hp_ctx *ctx, const float *pi_dev, const float *q_pi_dev, const double *actions_dev, const float *q_dev,
                            int64_t n_episodes, int32_t T, int32_t act_dim, double max_action, double sat, double *stats_dev);
int hp_episode_policy_stats_block(hp_rollout *ro, const float *pi_dev, const float *q_pi_dev, const float *q_dev,
                                  int64_t first_episode, int64_t n_episodes, double max_action, double sat, double *stats_dev);
int hp_episode_policy_summary(hp_ctx *ctx, const double *policy_stats_dev, int64_t n_episodes, double *summary_dev);

/* ---- actor-signal audit on the device ------------------------------------------------------------
 * The quantity that moves the actor, for every step of an episode block: a sample's actor update is dQ/da at a = pi(s), minus
 * the action_l2 pull, passed through tanh' (ddpg_agent.py:265-267 through the critic of models.py:28-44).  Where the critic is
 * flat in the action the actor learns nothing, or only shrinks towards zero under the regulariser; a demonstration helps only
 * where the gradient at pi(s) points towards the demonstrated action.
 *
 * hp_episode_action_grad: dq_du_dev[e][t][j] (float32) = d Q(s_t, u) / d u_j, u the critic's action input a / max_action, for
 * t = 0 .. T-1 of n_episodes episodes in ONE launch: an update's actor-side chain (same device functions, 4-row slabs) up to the
 * action columns of the critic's input gradient, seeded with dQ/dq = 1 for every row instead of an update's -1 / B.  dQ/da is
 * dq_du / max_action; it is not stored.  at 0: at the policy, u = (max_action * tanh) / max_action as hp_episode_policy forms it;
 * pi_dev[e][t][j] and q_dev[e][t] = Q(s_t, pi(s_t)) are hp_episode_policy's, bit for bit.  at 1: at the recorded action,
 * u = (float)actions[e][t][j] / max_action as hp_episode_q forms it; q_dev[e][t] = Q(s_t, a_t) is hp_episode_q's, bit for bit;
 * no actor runs and pi_dev is not written (it may be NULL; actions_dev may be NULL with at 0).  Arrays and clip_obs as for
 * hp_episode_policy / hp_episode_q.  target 0: the online networks.  target 1 is refused with HP_ERR_STATE: the target networks
 * keep no dX-order weight fragments (no update differentiates through them) and this call builds none.
 * hp_episode_action_grad_block is the same on episodes [first_episode, first_episode + n_episodes) of a block, whose recorded
 * actions it reads.  Both asynchronous on the context's stream (or a borrowed one), behind whatever wrote the weights; nothing
 * is allocated.  Refusals are hp_episode_policy's in its order, naming the entry point; behind target: at outside {0, 1}, at 1
 * without actions_dev, at 0 without pi_dev (HP_ERR_INVALID); behind the agent's shape: target 1 (HP_ERR_STATE).
 *
 * hp_episode_signal_stats: stats_dev [n][HP_SIGNAL_STATS] (float64) out of pi_dev and dq_du_dev (both of at 0) and the recorded
 * actions_dev [n][T][act_dim] (float64).  With M = (double)(float)max_action, lambda = action_l2, and per step g_j = dq_du[t][j],
 * v_j = pi[t][j] / M, d_j = (a[t][j] - pi[t][j]) / M, |x| = sqrt(sum_j x_j x_j):
 *   [0] grad_norm        sum_t |g| / T
 *   [1] flat_share       #{t : |g| < flat} / T
 *   [2] reg_share        #{t : (lambda * (2 / act_dim)) * |v| > |g|} / T: the regulariser outweighs the critic
 *   [3] toward_recorded  sum_t c_t / T, c_t = (sum_j g_j d_j) / (|g| * |d|), 0 where that product is 0
 *   [4] linear_adv       sum_t (sum_j g_j d_j) / T: the first-order estimate of Q(s, a) - Q(s, pi(s)), to be read beside
 *                        hp_episode_policy_stats' advantage_mean (which is Q(s, pi(s)) - Q(s, a))
 *   [5] trunk_signal     sum_t |s| / T, s_j = (g_j - ((lambda * 2) * v_j) / act_dim) * (1 - v_j v_j): what reaches the actor's
 *                        trunk behind the tanh, per sample
 * every float32 widened to float64, every sum started at 0 and accumulated in ascending t (inner j ascending), every operation
 * rounded on its own: the order is fixed and synthetic.episode_signal_stats is the same loop, so the bits are the host twin's.  One
 * wave per episode.  hp_episode_signal_stats_block takes the actions of a block's episodes.  hp_episode_signal_summary reduces
 * n_episodes rows to the six column means, left to right in episode order (synthetic.episode_signal_summary).  All asynchronous,
 * nothing allocated; HP_ERR_INVALID, naming the entry point, for a null argument, n_episodes or T out of range as for
 * hp_episode_stats, act_dim outside [1, HP_POLICY_MAX_ACT_DIM], max_action not positive and finite, action_l2 or flat negative or
 * not finite, episodes outside the block. */
#define HP_SIGNAL_STATS 6
int hp_episode_action_grad(hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t target, int32_t at, const double *obs_dev,
                           const double *g_dev, const double *actions_dev, int64_t n_episodes, int32_t T, double clip_obs,
                           float *pi_dev, float *q_dev, float *dq_du_dev);
int hp_episode_action_grad_block(hp_rollout *ro, hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t target, int32_t at,
                                 int64_t first_episode, int64_t n_episodes, double clip_obs, float *pi_dev, float *q_dev,
                                 float *dq_du_dev);
int hp_episode_signal_stats(hp_ctx *ctx, const float *pi_dev, const float *dq_du_dev, const double *actions_dev, int64_t n_episodes,
                            int32_t T, int32_t act_dim, double max_action, double action_l2, double flat, double *stats_dev);
int hp_episode_signal_stats_block(hp_rollout *ro, const float *pi_dev, const float *dq_du_dev, int64_t first_episode,
                                  int64_t n_episodes, double max_action, double action_l2, double flat, double *stats_dev);
int hp_episode_signal_summary(hp_ctx *ctx, const double *signal_stats_dev, int64_t n_episodes, double *summary_dev);

/* ---- Bellman audit on the device -----------------------------------------------------------------
 * The quantity the critic is trained on, for every step of an episode block: the residual of ddpg_agent.py:249-263,
 *   y_t = clamp(r_t + gamma Q'(s_{t+1}, pi'(s_{t+1})), -1 / (1 - gamma), 0),   delta_t = y_t - Q(s_t, a_t).
 * The critic audit sets Q beside the discounted return of the recorded episode, which for exploring episodes belongs to another
 * policy than the one the target bootstraps from; a critic can sit far from that return and still have no TD error.
 *
 * hp_episode_bellman: for t = 0 .. T-1 of n_episodes episodes in ONE launch (an update's target chain and its critic forward, same
 * device functions, 4-row slabs), all float32 [n][T]:
 *   q_next_dev  Q'(s_{t+1}, pi'(s_{t+1})): target actor, then target critic, on obs[e][t + 1] and the row's goal G(e, t), the action
 *               formed as (max_action * tanh) / max_action as hp_episode_policy forms it; pi' is not stored
 *   q_dev       Q(s_t, a_t): the online critic on obs[e][t], G(e, t) and the recorded action; with HP_GOAL_DESIRED hp_episode_q's bits
 *   r_dev       the reward of the transition under G(e, t): compute_reward on (ag[e][t + 1], G(e, t)), narrowed to float32 as the
 *               learner narrows it; distance_threshold and reward_type (0 sparse, 1 dense) as for hp_episode_returns
 *   y_dev       y = r + gamma * q_next; y = fminf(fmaxf(y, -clip_ret), 0) in float32, with the two float32 values the agent hands its
 *               own update kernels (gamma and 1 / (1 - gamma) of its configuration): an update's target for that row
 * goal_mode HP_GOAL_DESIRED: G(e, t) = g[e][t], the update's rule for an unrelabelled transition (g_next = g).  HP_GOAL_FINAL:
 * G(e, t) = ag[e][T] for every t, the episode's last achieved goal -- the relabel under which every episode ends in success; g_dev
 * is not read (it must still be given).  Arrays: obs_dev [n][T + 1][obs], ag_dev [n][T + 1][goal], g_dev [n][T][goal], actions_dev
 * [n][T][act], float64; clip_obs as for hp_episode_q.  hp_episode_bellman_block is the same on episodes [first_episode,
 * first_episode + n_episodes) of a block.  Both asynchronous on the context's stream (or a borrowed one), behind whatever wrote
 * the weights; no copy, nothing allocated.  Refusals are hp_episode_policy's in its order, naming the entry point (the agent's
 * shape: HP_ERR_STATE); behind the row count: goal_mode outside {0, 1}, then reward_type outside {0, 1} (HP_ERR_INVALID).
 *
 * hp_episode_bellman_stats: stats_dev [n][HP_BELLMAN_STATS] (float64) out of the four arrays.  With d_t = (double)y_t - (double)q_t:
 *   [0] td_mean        sum_t d_t / T
 *   [1] td_abs         sum_t |d_t| / T
 *   [2] td_sq          sum_t d_t d_t / T: the critic loss of these rows
 *   [3] target_mean    sum_t y_t / T
 *   [4] clipped_share  #{t : r_t + (float)gamma * q_next_t, in float32, is not y_t} / T: the steps whose clamp changed the value
 *   [5] reward_mean    sum_t r_t / T
 * every float32 widened to float64, every sum started at 0 and accumulated in ascending t, every operation rounded on its own:
 * synthetic.episode_bellman_stats is the same loop, so the bits are the host twin's.  gamma is narrowed to float32 as the agent
 * narrows its own.  One wave per episode.  hp_episode_bellman_summary reduces n_episodes rows to the six column means, left to
 * right in episode order (synthetic.episode_bellman_summary).  Asynchronous, nothing allocated; HP_ERR_INVALID, naming the entry
 * point, for a null argument, n_episodes or T out of range as for hp_episode_stats, gamma outside [0, 1]. */
#define HP_BELLMAN_STATS 6
#define HP_GOAL_DESIRED 0
#define HP_GOAL_FINAL 1
int hp_episode_bellman(hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t goal_mode, const double *obs_dev, const double *ag_dev,
                       const double *g_dev, const double *actions_dev, int64_t n_episodes, int32_t T, double distance_threshold,
                       int32_t reward_type, double clip_obs, float *q_dev, float *q_next_dev, float *r_dev, float *y_dev);
int hp_episode_bellman_block(hp_rollout *ro, hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm, int32_t goal_mode, int64_t first_episode,
                             int64_t n_episodes, double distance_threshold, int32_t reward_type, double clip_obs, float *q_dev,
                             float *q_next_dev, float *r_dev, float *y_dev);
int hp_episode_bellman_stats(hp_ctx *ctx, const float *q_dev, const float *q_next_dev, const float *r_dev, const float *y_dev,
                             int64_t n_episodes, int32_t T, double gamma, double *stats_dev);
int hp_episode_bellman_summary(hp_ctx *ctx, const double *bellman_stats_dev, int64_t n_episodes, double *summary_dev);

/* Policy calls that do not queue behind training: hp_agent_policy_snapshot copies the online actor and both normalizers'
 * statistics (stream-ordered with the updates, no host wait); hp_agent_act_snapshot evaluates the most recent COMPLETE
 * snapshot on a second stream, so a feeder can step its environments while a training cycle runs (its policy lags the
 * learner by at most one snapshot interval; the reference's rollouts are synchronous, ddpg_agent.py:101-150).  Same
 * arithmetic as hp_agent_act.  Callable from another host thread. */
int hp_agent_policy_snapshot(hp_agent *ag, hp_norm *o_norm, hp_norm *g_norm);
int hp_agent_act_snapshot(hp_agent *ag, const double *obs_host, const double *g_host, int64_t rows, double clip_obs,
                          float *actions_host);

/* Split-phase update for data-parallel ranks (utils.sync_grads, utils.py:43-48):
 *   forward_backward: sample + forwards + backwards, leaves SUM-able gradients in one flat device
 *   vector (*dev_grads, both nets, padded layout -- every rank has the same layout);
 *   apply: Adam on whatever that vector holds after the caller's all-reduce. */
int hp_agent_forward_backward(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng,
                              double future_p, double sq_threshold);
int hp_agent_grad_buffer(hp_agent *ag, void **dev_grads, int64_t *n_floats);
int hp_agent_param_buffer(hp_agent *ag, void **dev_params, int64_t *n_floats); /* actor|critic, for Bcast (utils.py:6-15) */
int hp_agent_apply(hp_agent *ag);
/* ddpg_agent.py:33-34: targets := online nets.  Also the call that makes parameters written through
 * hp_agent_param_buffer (broadcast from rank 0) take effect in the kernels' weight copies. */
int hp_agent_sync_targets(hp_agent *ag);

/* ---- rank exchange on RCCL (one process per GPU; replaces mpi4py) -------------------------------
 * The three exchanges of the reference: sync_networks (utils.py:6-15, Bcast from rank 0), sync_grads
 * (utils.py:43-48, Allreduce SUM of the flat gradients, every update) and the normalizer's
 * _mpi_average (normalizer.py:60-64, Allreduce SUM / size).  Bootstrap: rank 0 calls
 * hp_comm_unique_id, the 128 bytes travel to the other ranks by any side channel (the Python mirror
 * uses torch.distributed), every rank calls hp_comm_create.  Collectives are enqueued on the
 * context's stream.  RCCL is resolved with dlopen at first use; without it these return HP_ERR_STATE. */
int hp_comm_unique_id(uint8_t *out128);
int hp_comm_create(hp_ctx *ctx, const uint8_t *id128, int32_t rank, int32_t world, hp_comm **out);
int hp_comm_info(hp_comm *comm, int32_t *rank, int32_t *world);
int hp_comm_allreduce_sum_f32(hp_comm *comm, void *dev, int64_t n);    /* in place, device pointer */
int hp_comm_allreduce_mean_f32(hp_comm *comm, void *dev, int64_t n);   /* SUM then / world (float32) */
int hp_comm_broadcast_f32(hp_comm *comm, void *dev, int64_t n, int32_t root);
void hp_comm_destroy(hp_comm *comm);
/* Attach (or detach with NULL) a communicator: hp_agent_sample_and_update and hp_agent_train_cycle then
 * all-reduce the gradients between backward and Adam inside the library (and train_cycle the
 * normalizer sums), so the data-parallel loop needs no host round trip per update and stays inside
 * the cycle's hipGraph.  The split-phase calls above keep working for callers with their own transport. */
int hp_agent_set_comm(hp_agent *ag, hp_comm *comm);
/* Reduction applied to the gradients when a communicator is attached: 0 (default) = SUM, exactly utils.py:47 -- N
 * ranks therefore step with N times the single-rank gradient; 1 = MEAN (SUM / world size), for callers who want the
 * learning rate to keep its single-rank meaning at a larger global batch. */
int hp_agent_set_grad_reduce(hp_agent *ag, int32_t mean);
/* diagnostic: 0 = no cycle built yet, 1 = hp_agent_train_cycle replays a cached hipGraph, 2 = it issues eager
 * launches because a capture containing collectives was refused by the runtime */
int hp_agent_cycle_mode(hp_agent *ag, int32_t *mode);

/* ---- rank exchange as one-shot all-reduces over peer memory (xGMI), fused with the optimizer ----------------------------
 * Same three exchanges as above, but without a collective library on the critical path of an update: every rank exports
 * one block of exchange memory (hipIpcGetMemHandle), maps the other ranks' blocks, and the kernel that applies Adam
 * reads the peers' gradient vectors itself and sums them in rank order (utils.py:43-48 SUM; bit-identical parameters on
 * every rank).  Bootstrap: hp_peer_create on every rank -> exchange the 64-byte handles through any side channel ->
 * hp_peer_connect(all handles, rank order).  Waits are bounded (RLARM_PEER_TIMEOUT_S, default 20 s) and a timeout is FATAL
 * for the exchange: the kernel whose wait gave up skips its sum / optimizer step, sets a sticky error word that makes every
 * later exchange kernel return at once, and mirrors it into pinned host memory -- hp_agent_train_cycle /
 * hp_agent_sample_and_update then fail with HP_ERR_STATE at their next call (no synchronisation needed), hp_peer_status
 * reads the word explicitly.  The reference's MPI Allreduce (utils.py:47) would block forever instead; silent divergence of
 * the replicas is the one outcome that is excluded.  One node only (ranks that can map each other's device memory). */
int hp_peer_create(hp_ctx *ctx, int32_t rank, int32_t world, int64_t n_grad_floats, hp_peer **out, uint8_t *handle64);
int hp_peer_connect(hp_peer *peer, const uint8_t *handles_world_x_64);
/* normalizer._mpi_average (normalizer.py:60-64) and other small vectors (<= 1024 floats): in place, SUM or SUM / world
 * (mean != 0), enqueued on the context's stream; collective */
int hp_peer_allreduce_f32(hp_peer *peer, void *dev, int64_t n, int32_t mean);
/* collective self-check of the gradient channel (flags, both buffer parities, system-scope loads of every peer's vector) on an
 * exactly representable pattern: *mismatches = number of wrong elements on this rank (top bit: a wait timed out) */
int hp_peer_selfcheck(hp_peer *peer, uint32_t *mismatches);
int hp_peer_status(hp_peer *peer, uint32_t *error);
/* Gate mode (every rank alike, before the first exchange): each wait of the gradient exchange runs in a ONE-WAVEFRONT kernel
 * of its own in front of the kernel that consumes the peers' data, instead of inside that kernel's hundreds of workgroups.
 * Needed when ranks share one physical device (rehearsals of an N-GPU job on one GPU): there a rank's progress depends on
 * its kernels being co-resident with the other ranks' WAITING kernels, and workgroups spinning by the hundred can starve
 * them of registers / LDS.  Costs one kernel boundary per wait; default off. */
int hp_peer_set_gate(hp_peer *peer, int32_t on);
/* 1: one-shot exchange (every rank reads every peer's whole gradient vector), 2: reduce-scatter + all-gather over the same
 * peer memory (default from 4 ranks; RLARM_PEER_PHASES=1|2).  Both sum in rank order: bit-identical results. */
int hp_peer_phases(hp_peer *p, int32_t *phases);
void hp_peer_destroy(hp_peer *peer);
/* Attach (or detach with NULL): hp_agent_sample_and_update / hp_agent_train_cycle then exchange the gradients through
 * peer memory inside the optimizer kernel and the normalizer sums through the mailboxes.  hp_agent_grad_buffer-style
 * host-driven exchange keeps working.  n_grad_floats of the peer must equal hp_agent_grad_buffer's length. */
int hp_agent_set_peer(hp_agent *ag, hp_peer *peer);

/* One training cycle's learner half (ddpg_agent.py:143-150) as one cached hipGraph:
 *   store n_new episodes -> update normalizers (+recompute) -> n_batches updates -> soft update.
 * Requires single-rank operation (no cross-rank exchange inside the graph). Asynchronous. */
int hp_agent_train_cycle(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng,
                         const double *obs, const double *ag_host, const double *g, const double *actions,
                         int64_t n_new, double future_p, double sq_threshold, int32_t n_batches);
/* The same cycle (ddpg_agent.py:143-150) on episodes that lie in a host block registered with the device (hp_host_register;
 * layout and ticket as hp_buffer_store_pinned): what a multi-process rollout feeder (ddpg_agent.py:101-144 spread over worker
 * processes) calls per wave -- the store is an asynchronous DMA out of the shared ring, no CPU copy. */
int hp_agent_train_cycle_pinned(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng,
                                const double *block, int64_t n_new, double future_p, double sq_threshold,
                                int32_t n_batches, uint64_t *ticket);
/* ... and on a block in device memory (hp_rollout_block): no DMA from the host, no ticket; same launches otherwise. */
int hp_agent_train_cycle_dev(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng,
                             const double *block_dev, int64_t n_new, double future_p, double sq_threshold,
                             int32_t n_batches);

/* ---- training state: stop a run and continue it bit for bit ---------------------------------------------
 * What the reference wished for and never finished (ddpg_agent.py:54-62, "load the data to continue the training", commented
 * out; its save_checkpoint :158-161 keeps the normalizer statistics and the actor only).  A training state is everything the
 * learner's future depends on, in `n` named sections of one byte blob (hp_state_layout):
 *   actor, critic, actor_target, critic_target, adam_{actor,critic}_{m,v}   float32, the reference's flat named_parameters()
 *       order (utils.py:18-27) -- converted from / to the padded arena on the device, so a blob does not depend on engine, slab
 *       width or RLARM_* switches;           adam_step  int64 [1] (both optimizers step together)
 *   {o,g}_norm_{local_sum,local_sumsq,local_count,total_sum,total_sumsq,total_count,mean,std}   normalizer.py:12-20, all of it
 *   rng_key uint32 [624], rng_pos int32 [1]   the MT19937 stream (np.random.get_state()[1:3])
 *   buffer_{obs,ag,g,actions}   float64 rows of episodes [0, current_size), slot order;   buffer_counters  int64 [2] =
 *       current_size, n_transitions_stored (replay_buffer.py:18-19)
 * NOT part of a state: staged episodes (hp_buffer_stage), sampling plans, gradients, the loss log -- after a restore
 * hp_agent_get_losses reports only updates made since --, policy snapshots (hp_agent_policy_snapshot must be called again before
 * hp_agent_act_snapshot) and the profiling state.
 * Checksum of a section: its bytes as little-endian 64-bit words w_0 .. w_{n-1} (the last zero-padded to 8 bytes),
 * A = sum w_i mod 2^64, B = sum (i + 1) w_i mod 2^64.  sums[2 i], sums[2 i + 1] = (A, B) of section i. */
typedef struct {
    char name[32];
    int32_t dtype;        /* 0 float32, 1 float64, 2 int64, 3 uint32, 4 int32 */
    int32_t elem_bytes;
    int64_t count;        /* elements */
    int64_t offset;       /* bytes from the start of the blob (a multiple of 256) */
} hp_state_section;
typedef struct {          /* shapes a state was captured with: hp_state_restore compares them with the receiving objects */
    int32_t obs_dim, goal_dim, act_dim, hidden, T, reserved;
    int64_t capacity;     /* hp_buffer_create's size_episodes: overflow slot draws depend on it (replay_buffer.py:57-71) */
    int64_t current_size; /* episodes the blob holds */
} hp_state_dims;
#define HP_STATE_SECTIONS 32
/* Sections of a state of `current_size` episodes (< 0: what the buffer holds now) for these objects.  out may be NULL; *n: in, room
 * in out; out, HP_STATE_SECTIONS.  *total_bytes: size of the blob. */
int hp_state_layout(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, int64_t current_size, hp_state_section *out,
                    int32_t *n, size_t *total_bytes);
/* Snapshot, stream-ordered, without a host wait: the context's stream gets device-to-device copies of every section into an arena
 * the agent owns (grown when needed) and an event; a second stream waits for the event, sums every section and drains arena and sums
 * to pinned host memory in chunks.  The learner's next call (hp_agent_train_cycle, ...) may follow at once: it neither waits for the
 * drain nor can it alter what the drain reads.  One capture at a time: while a ticket has not been fetched, a second capture FAILS
 * with HP_ERR_STATE (nothing enqueued).  *bytes (may be NULL): size of the blob hp_state_fetch will deliver. */
int hp_state_capture(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng, uint64_t *ticket, size_t *bytes);
/* Collect a capture: wait != 0 blocks until the drain is over (outside the context's lock: another thread keeps training), else
 * *done = 0 is returned while it runs.  Then the blob is copied to host_out (`bytes` must be the capture's size), sums[2 *
 * HP_STATE_SECTIONS] receives the device-side checksums, the ticket is retired and *done = 1.  host_out == NULL abandons the
 * ticket (waits for its drain).  One thread per ticket. */
int hp_state_fetch(hp_agent *ag, uint64_t ticket, int32_t wait, void *host_out, size_t bytes, uint64_t *sums, int32_t *done);
/* Put a state back -- into fresh objects or into ones that have run since (roll-back; cached update and cycle graphs stay
 * valid).  dims that differ from the receivers are refused with HP_ERR_INVALID and a message naming the field.  The blob is uploaded
 * into the snapshot arena and summed THERE; sums that differ from `sums` are refused with HP_ERR_INVALID naming the section BEFORE
 * any live state is touched.  Then: parameters, targets, Adam m / v / step, both normalizers, the random stream, buffer rows into
 * the same slots, the counters on the device and in the host mirror; the kernels' weight copies are rebuilt as hp_agent_set_params
 * does, the float32 throughput rows when the buffer has them.  Synchronises. */
int hp_state_restore(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng, const hp_state_dims *dims,
                     const void *host_in, size_t bytes, const uint64_t *sums);
/* ---- delta states: the buffer as the episodes written since a base capture -----------------------------------
 * The buffer keeps a uint32 stamp per slot and one device word, the capture epoch (1 at creation).  Every scatter of an episode
 * (hp_buffer_store*, hp_agent_train_cycle*, eager or inside a cached graph) stamps its slot with the epoch it READS from device
 * memory; every capture, full or delta, records `capture_epoch = epoch` in stream order and then advances the epoch.  Stamps are
 * absolute: a slot is dirty with respect to a capture c iff its stamp is > c, so a capture that is never fetched loses nothing.
 * hp_state_restore zeroes the stamps, makes `min_since` a value larger than any epoch handed out before and leaves the epoch at
 * min_since + 1: the restored state itself stands for a capture with epoch min_since.
 * A delta blob has HP_STATE_DELTA_SECTIONS sections: the 27 small ones of a full state (actor .. rng_pos) under the same names, then
 *   buffer_delta_header  int64 [4] = n_dirty, overflow, capture_epoch, since_epoch
 *   buffer_delta_slots   int64 [max_dirty]: the slots in [0, current_size) with stamp > since_epoch, ascending; n_dirty are used
 *   buffer_delta_{obs,ag,g,actions}   float64 [max_dirty][...]: the rows of those slots, in that order; n_dirty episodes are used
 *   buffer_counters      int64 [2]
 * The slot and row sections are summed over their used prefix. */
#define HP_STATE_DELTA_SECTIONS 34
/* Sections of a delta sized for `max_dirty` episodes.  out may be NULL; *n: in, room in out; out, HP_STATE_DELTA_SECTIONS. */
int hp_state_layout_delta(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, int64_t max_dirty, hp_state_section *out,
                          int32_t *n, size_t *total_bytes);
/* As hp_state_capture, with the buffer captured as the slots written since the capture `since_epoch` (dirty scan + row pack on the
 * context's stream).  max_dirty in [0, current_size] bounds the episodes the blob has room for: the caller passes min(episodes
 * stored since that capture, current_size).  since_epoch below the buffer's min_since, or not below its epoch, is refused with
 * HP_ERR_STATE before anything is enqueued.  Shares the one-capture-at-a-time rule and hp_state_fetch with hp_state_capture; the
 * `sums` given to hp_state_fetch must then hold 2 * HP_STATE_DELTA_SECTIONS words.  A delta that found more than max_dirty dirty
 * slots makes hp_state_fetch fail with HP_ERR_STATE (the ticket is retired, nothing is delivered). */
int hp_state_capture_delta(hp_agent *ag, hp_buffer *buf, hp_norm *o_norm, hp_norm *g_norm, hp_rng *rng, uint32_t since_epoch,
                           int64_t max_dirty, uint64_t *ticket, size_t *bytes);
/* The epochs, from the host mirror (no wait): *capture_epoch = what this agent's most recent capture recorded (0: none yet),
 * *epoch = the buffer's current epoch, *min_since = the smallest since_epoch a delta capture accepts.  Any pointer may be NULL. */
int hp_state_epochs(hp_agent *ag, hp_buffer *buf, uint32_t *capture_epoch, uint32_t *epoch, uint32_t *min_since);
/* The checksum kernel on any device memory (8-byte aligned): out2 = (A, B).  blocks = 0: the library's grid, else that many
 * workgroups (the result does not depend on it).  Synchronises. */
int hp_state_checksum_dev(hp_ctx *ctx, const void *dev, size_t bytes, int32_t blocks, uint64_t *out2);

/* timing hook for bench.py: average device time (ms) of the kernels tagged `which` over the
 * last recorded region; see DESIGN.md "Measurement". */
/* Which kernels hp_agent_sample_and_update / hp_agent_train_cycle run for this agent (chosen at creation from the batch
 * size and the RLARM_* switches): *engine = 0 layer-per-launch, 8 thin row slabs (slab8.h, *slab_rows = 4 / 8 / 16),
 * 32 the 32-row engine (slab32.h); *dw_split = 0 for 32 x 32 weight-gradient tiles
 * (gemm_lds.h), else the number of batch-row slices per 64 x 64 tile (dw64.h).  Any pointer may be null. */
int hp_agent_engine(hp_agent *ag, int32_t *engine, int32_t *slab_rows, int32_t *dw_split);
/* Launch structure of a sequence of n_updates sampled updates WITH their optimizer steps (ddpg_agent.py:145-147;
 * hp_agent_sample_and_update, hp_agent_train_cycle) on this agent as it is now: *form = 0 chain launch + weight-gradient launch per
 * update; 1 split launch (target networks one update ahead, the critic's weight gradients inside the chain launch) + the actor's
 * weight-gradient launch -- single rank: optimizer steps in both launches' epilogues; data-parallel ranks on a device each: the same
 * with the tile-wise rank exchange in front of every step, or gradients only + exchange + optimizer launches (RCCL, two-phase
 * peer memory).  Gradient-only calls (hp_agent_forward_backward) always take form 0.  The kernels by name:
 * hp_agent_update_kernels (rlarm_hip_debug.h). */
int hp_agent_update_form(hp_agent *ag, int32_t n_updates, int32_t *form);
/* Sticky health word of the learner, free for the host (pinned memory, no synchronisation): 0 = healthy.  Bit 0: a bounded
 * in-launch hand-off gave up; one bit per source beside it (several may be set): bit 4 critic chains -> weight-gradient tiles,
 * bit 5 actor chains -> critic optimizer step, bit 6 cycle-opening launch; the launches since skipped work, every later hp_agent_train_cycle* /
 * hp_agent_sample_and_update / hp_agent_get_losses fails with HP_ERR_STATE, the agent must be recreated. */
int hp_agent_status(hp_agent *ag, uint32_t *fault);
int hp_agent_profile(hp_agent *ag, int32_t enable);
int hp_agent_profile_read(hp_agent *ag, double *ms_out, int32_t n);

void hp_agent_destroy(hp_agent *ag);
void hp_norm_destroy(hp_norm *nz);
void hp_buffer_destroy(hp_buffer *buf);

#ifdef __cplusplus
}
#endif
#endif /* RLARM_HIP_H */
