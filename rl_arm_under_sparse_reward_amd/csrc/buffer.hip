// buffer.hip -- episodic replay storage in HBM: staging and storing episodes, the throughput rows, reading back, and the goal
// reward ops (reference: replay_buffer.py:11-71, bmirobot_env_push_F.py:20-23,84-90).  Sampling from it: sampler.hip.
//
// HBM layout (float64, identical to the reference's numpy arrays so that episodes can be
// memcpy'd in and read back verbatim):
//   obs  [size][T+1][obs_dim]   ag [size][T+1][goal_dim]
//   g    [size][T][goal_dim]    actions [size][T][act_dim]
#include "store_device.h"
#include "transition_device.h"

#include <cmath>

// ----------------------------------------------------------------------------- kernels
// ---- throughput rows (SURVEY 8b storage_dtype = fp32; hp_buffer_enable_f32_rows / hp_buffer_sample_dev_f32) -----------------------
// The float64 arrays above are the reference's layout and stay the source of truth.  The mirror below is laid out for the
// gather instead: one (episode, timestep) = ONE 128-byte line of float32 [obs_t | action_t | 0], so a transition's
// observations and action are two adjacent, line-aligned lines (the float64 rows are a 432-byte run at any 8-byte offset:
// 4.4 lines, plus a line for the action); the goals stay float64 -- the reward and the relabelled goal are bit-exact as before --
// as [ag_t | g_t | 0] per 64 bytes, so ag[t + 1] and g[t] share 128 bytes.  PMC, 2^18 transitions: 947 B fetched per transition
// from the float64 rows (7.4 lines), 5xx from these.  Observations and actions are rounded to float32 at store time (actions
// lose nothing the learner sees: it consumes float32(actions)); the normaliser arithmetic on them is unchanged (float64).
__global__ __launch_bounds__(256) void k_pack_rows(const long long *__restrict__ slots, long long n, long long first,
                                                   const double *__restrict__ obs, const double *__restrict__ ag,
                                                   const double *__restrict__ g, const double *__restrict__ act, float *p_row,
                                                   double *p_goal, int T, int od, int gd, int ad, int row_w, int goal_w) {
    // one workgroup per (episode, block of 8 timesteps); slots == nullptr: episodes first .. first + n - 1
    const long long i = blockIdx.x / ((T + 8) / 8);
    const int t0 = (int)(blockIdx.x % ((T + 8) / 8)) * 8;
    const long long e = slots ? slots[i] : first + i;
    for (int idx = threadIdx.x; idx < 8 * row_w; idx += blockDim.x) {
        const int t = t0 + idx / row_w, c = idx % row_w;
        if (t > T) continue;
        float v = 0.f;
        if (c < od) v = (float)obs[(e * (T + 1) + t) * od + c];
        else if (c < od + ad && t < T) v = (float)act[(e * T + t) * ad + (c - od)];
        p_row[(e * (T + 1) + t) * row_w + c] = v;
    }
    for (int idx = threadIdx.x; idx < 8 * goal_w; idx += blockDim.x) {
        const int t = t0 + idx / goal_w, c = idx % goal_w;
        if (t > T) continue;
        double v = 0.0;
        if (c < gd) v = ag[(e * (T + 1) + t) * gd + c];
        else if (c < 2 * gd && t < T) v = g[(e * T + t) * gd + (c - gd)];
        p_goal[(e * (T + 1) + t) * goal_w + c] = v;
    }
}

// Batched compute_reward / _is_success of the bmirobot GoalEnvs (bmirobot_env_push_F.py:84-90, :243-245; identical in
// bmirobot_env_pickandplace_v2.py) on device arrays [n][goal_dim] float64.  mode 0: sparse reward -(d > thr) as float32
// (bits 0x80000000 / 0xBF800000); mode 1: dense reward -d as float64; mode 2: success (d < thr) as float32.
// thr_sq = the squared-domain threshold of the predicate (see hp_compute_reward); no square root in modes 0 and 2.
__global__ __launch_bounds__(256) void k_goal_reward(const double *__restrict__ ag, const double *__restrict__ g,
                                                     long long n, int goal_dim, double thr_sq, int mode, float *out32,
                                                     double *out64) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double s = tr_sq_distance(ag + i * goal_dim, g + i * goal_dim, goal_dim);
    if (mode == 0) out32[i] = (s >= thr_sq) ? -1.0f : -0.0f;
    else if (mode == 1) out64[i] = -__dsqrt_rn(s);
    else out32[i] = (s < thr_sq) ? 1.0f : 0.0f;
}

// scatter the staged episodes into their slots.  numpy's `buffers[idxs] = mb` lets the LAST
// occurrence of a repeated slot win, so an episode is dropped when a later one has its slot.
#define STORE_PARTS 8
__global__ __launch_bounds__(256) void k_store_scatter(const long long *__restrict__ slots, long long n_new,
                                                       const double *s_obs, const double *s_ag, const double *s_g,
                                                       const double *s_act, double *obs, double *ag, double *g,
                                                       double *act, long long ep_obs, long long ep_ag,
                                                       long long ep_g, long long ep_act, uint32_t *slot_epoch,
                                                       const uint32_t *epoch) {
    // STORE_PARTS workgroups per episode, each a strided share of its values: one or two copies per thread instead of a
    // loop of fifteen dependent-latency iterations (the copy of 2 episodes was 9.6 us of every cycle)
    store_scatter_share([&](long long j) { return slots[j]; }, blockIdx.x / STORE_PARTS, blockIdx.x % STORE_PARTS, STORE_PARTS,
                        n_new, s_obs, s_ag, s_g, s_act, obs, ag, g, act, ep_obs, ep_ag, ep_g, ep_act, slot_epoch, epoch);
}

// ------------------------------------------------------------------------------ launchers
// throughput rows of the episodes in st_slots[0 .. n_new) (just scattered) -- or, slots == nullptr, of episodes [first, first + n)
static int launch_pack(hp_buffer *b, const long long *slots, int64_t first, int64_t n) {
    if (!b->p_row || n <= 0) return HP_OK;
    const unsigned per_ep = (unsigned)((b->T + 8) / 8);
    HP_KLOG("k_pack_rows");
    // ADVICE buffer.hip:1007 -- the guard on n * per_ep (and "pack only [0, current_size)") goes here
    hipLaunchKernelGGL(k_pack_rows, dim3((unsigned)n * per_ep), dim3(256), 0, b->ctx->stream, slots, (long long)n, (long long)first,
                       b->d_obs, b->d_ag, b->d_g, b->d_act, b->p_row, b->p_goal, (int)b->T, (int)b->obs_dim, (int)b->goal_dim,
                       (int)b->act_dim, (int)b->row_w, (int)b->goal_w);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}
int buffer_launch_pack(hp_buffer *b, int64_t n_new) { return launch_pack(b, b->st_slots.as<long long>(), 0, n_new); }
int buffer_launch_pack_range(hp_buffer *b, int64_t first, int64_t n) { return launch_pack(b, nullptr, first, n); }

// grow a staging allocation; moving it invalidates the captured cycles that read it (hp_buffer::gen)
static int stage_ensure(hp_buffer *b, DevBuf &d, size_t need) {
    if (need > d.bytes) ++b->gen;
    return d.ensure(need);
}

// the staging block (st_obs .. st_act) for n_new episodes, obs | ag | g | actions back to back; *n: the bytes of each and of all
static int stage_carve(hp_buffer *b, int64_t n_new, StageBytes *n) {
    *n = stage_bytes_of(n_new, b->ep_obs(), b->ep_ag(), b->ep_g(), b->ep_act());
    HP_TRY(stage_ensure(b, b->st_obs, n->total));
    char *dst = b->st_obs.as<char>();
    b->st_ag = reinterpret_cast<double *>(dst + n->at_ag());
    b->st_g = reinterpret_cast<double *>(dst + n->at_g());
    b->st_act = reinterpret_cast<double *>(dst + n->at_act());
    return HP_OK;
}
// the caller's four arrays into a host block of that layout
static void stage_fill_host(char *h, const StageBytes &n, const double *obs, const double *ag, const double *g, const double *actions) {
    memcpy(h, obs, n.obs);
    memcpy(h + n.at_ag(), ag, n.ag);
    memcpy(h + n.at_g(), g, n.g);
    memcpy(h + n.at_act(), actions, n.act);
}

// slots, scatter and throughput rows of the n_new staged episodes
static int store_staged(hp_buffer *b, hp_rng *rng, int64_t n_new) {
    HP_TRY(rng_launch_slots(rng, b, n_new, b->st_slots.as<int64_t>()));
    hipLaunchKernelGGL(k_store_scatter, dim3((unsigned)(n_new * STORE_PARTS)), dim3(256), 0, b->ctx->stream,
                       b->st_slots.as<long long>(), (long long)n_new, b->st_obs.as<double>(), b->st_ag, b->st_g, b->st_act, b->d_obs,
                       b->d_ag, b->d_g, b->d_act, (long long)b->ep_obs(), (long long)b->ep_ag(), (long long)b->ep_g(),
                       (long long)b->ep_act(), b->d_slot_epoch, b->d_epoch);
    HP_CHECK_HIP(hipGetLastError());
    return buffer_launch_pack(b, n_new);
}

// host mirror of replay_buffer.py:68 and :43
static void mirror_stored(hp_buffer *b, int64_t n_new) {
    b->current_size = (b->current_size + n_new < b->size) ? b->current_size + n_new : b->size;
    b->n_transitions_stored += (int64_t)b->T * n_new;
}

// stage host episodes on the device (st_*): one pinned copy, one H2D.  copy-in semantics (replay_buffer.py:39-42): the
// caller's arrays are read by the CPU memcpy below and never again; the DMA reads our pinned staging.
static int buffer_stage(hp_buffer *b, const double *obs, const double *ag, const double *g, const double *actions,
                        int64_t n_new) {
    hipStream_t s = b->ctx->stream;
    StageBytes n;
    HP_TRY(stage_carve(b, n_new, &n));
    HP_TRY(b->pin.ensure(n.total));
    stage_fill_host(static_cast<char *>(b->pin.p), n, obs, ag, g, actions);
    HP_CHECK_HIP(hipMemcpyAsync(b->st_obs.p, b->pin.p, n.total, hipMemcpyHostToDevice, s));
    HP_TRY(b->pin.mark(s));
    b->staged_n = n_new;
    b->ring_cur = -1;
    return HP_OK;
}

// stage, pick slots, scatter.  Shared by hp_buffer_store and the train-cycle path.
int buffer_stage_and_store(hp_buffer *b, hp_rng *rng, const double *obs, const double *ag, const double *g,
                           const double *actions, int64_t n_new) {
    HP_TRY(stage_ensure(b, b->st_slots, n_new * 8));
    HP_TRY(buffer_stage(b, obs, ag, g, actions, n_new));
    HP_TRY(store_staged(b, rng, n_new));
    mirror_stored(b, n_new);
    return HP_OK;
}

// Episodes in ONE block laid out obs | ag | g | actions back to back: an asynchronous copy of `kind` into the staging, and --
// store_now -- slots + scatter; without store_now those follow in the cycle's opening launch (hp_agent_train_cycle_pinned / _dev).
// ticket != nullptr: an event behind the copy, its number in *ticket.
static int stage_block(hp_buffer *b, hp_rng *rng, const double *block, hipMemcpyKind kind, int64_t n_new, uint64_t *ticket,
                       bool store_now) {
    hipStream_t s = b->ctx->stream;
    StageBytes n;
    HP_TRY(stage_ensure(b, b->st_slots, n_new * 8));
    HP_TRY(stage_carve(b, n_new, &n));
    HP_CHECK_HIP(hipMemcpyAsync(b->st_obs.p, block, n.total, kind, s));
    if (ticket) {
        // from a small ring (a ticket older than the ring is done by construction: its event is re-recorded only after this call
        // synchronised on it)
        const uint64_t t = ++b->pin_tickets;
        hipEvent_t &ev = b->pin_events[t % hp_buffer::PIN_RING];
        if (!ev) HP_CHECK_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        else HP_CHECK_HIP(hipEventSynchronize(ev));
        HP_CHECK_HIP(hipEventRecord(ev, s));
        *ticket = t;
    }
    b->staged_n = n_new;
    b->ring_cur = -1;
    if (store_now) HP_TRY(store_staged(b, rng, n_new));
    mirror_stored(b, n_new);
    return HP_OK;
}
// ... in a host block registered with the device (hp_host_register: the feeder's shared-memory ring): a DMA with a ticket behind it,
// taken whether or not the caller asks for its number
int buffer_stage_pinned(hp_buffer *b, hp_rng *rng, const double *block, int64_t n_new, uint64_t *ticket, bool store_now) {
    uint64_t unasked;
    return stage_block(b, rng, block, hipMemcpyHostToDevice, n_new, ticket ? ticket : &unasked, store_now);
}
// ... in a device block (hp_rollout's wave block): device to device, in stream order behind the kernels that wrote the block -- no
// DMA from the host, no ticket
int buffer_stage_dev(hp_buffer *b, hp_rng *rng, const double *block_dev, int64_t n_new, bool store_now) {
    return stage_block(b, rng, block_dev, hipMemcpyDeviceToDevice, n_new, nullptr, store_now);
}

// direct form: the episodes go as far as a block of the pinned ring; k_cycle_open loads them from there and fills st_* itself
static int buffer_stage_ring(hp_buffer *b, const double *obs, const double *ag, const double *g, const double *actions,
                             int64_t n_new) {
    StageBytes n;
    HP_TRY(stage_carve(b, n_new, &n));
    HipStageApi api;
    int idx = -1;
    bool moved = false;
    HP_TRY(b->ring.acquire(api, n.total, &idx, &moved));   // waits for the launch that last read this block
    if (moved) ++b->gen;
    stage_fill_host(static_cast<char *>(b->ring.slot[idx].host), n, obs, ag, g, actions);
    b->staged_n = n_new;
    b->ring_cur = idx;
    return HP_OK;
}

// the ring block of the cycle just enqueued may be overwritten once that cycle's opening launch has run.  The cycle IS enqueued
// when this is called: if the fence cannot be placed, the stream is drained instead, so the block is never left readable by a
// queued launch and unfenced; the failure is still reported.
int buffer_mark_cycle_block(hp_buffer *b) {
    if (b->ring_cur < 0) return HP_OK;
    HipStageApi api;
    const int st = b->ring.mark(api, b->ring_cur, b->ctx->stream);
    if (st != HP_OK) (void)hipStreamSynchronize(b->ctx->stream);
    return st;
}

int buffer_stage_for_cycle(hp_buffer *b, const double *obs, const double *ag, const double *g, const double *actions,
                           int64_t n_new, bool direct) {
    HP_TRY(stage_ensure(b, b->st_slots, n_new * 8));
    if (direct) HP_TRY(buffer_stage_ring(b, obs, ag, g, actions, n_new));
    else HP_TRY(buffer_stage(b, obs, ag, g, actions, n_new));
    mirror_stored(b, n_new);
    return HP_OK;
}

// what every store entry asks of n_new, under the context's lock
static int store_check(hp_buffer *b, int64_t n_new, const char *who) {
    HP_REQUIRE(n_new > 0, HP_ERR_INVALID, "%s: n_new must be positive", who);
    // replay_buffer.py:64 with current_size == 0 and inc > size: np.random.randint(0, 0, k) raises
    HP_REQUIRE(!(b->current_size == 0 && n_new > b->size), HP_ERR_INVALID, "high <= 0");
    return HP_OK;
}

// --------------------------------------------------------------------------------- C ABI
extern "C" {

int hp_buffer_create(hp_ctx *ctx, int64_t size_episodes, int32_t T, int32_t obs_dim, int32_t goal_dim,
                     int32_t act_dim, hp_buffer **out) {
    HP_REQUIRE(ctx && out, HP_ERR_INVALID, "hp_buffer_create: null argument");
    HP_REQUIRE(size_episodes > 0 && size_episodes < (1ll << 31), HP_ERR_INVALID,
               "hp_buffer_create: size_episodes=%lld must be in [1, 2^31)", (long long)size_episodes);
    HP_REQUIRE(T > 0 && obs_dim > 0 && goal_dim > 0 && act_dim > 0, HP_ERR_INVALID,
               "hp_buffer_create: dimensions must be positive");
    hp_buffer *b = new hp_buffer();
    b->ctx = ctx;
    b->size = size_episodes;
    b->T = T;
    b->obs_dim = obs_dim;
    b->goal_dim = goal_dim;
    b->act_dim = act_dim;
    hipError_t e = hipSuccess;
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_obs, size_episodes * b->ep_obs() * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_ag, size_episodes * b->ep_ag() * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_g, size_episodes * b->ep_g() * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_act, size_episodes * b->ep_act() * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_meta, sizeof(BufMeta));
    if (e == hipSuccess) e = hipMemsetAsync(b->d_meta, 0, sizeof(BufMeta), ctx->stream);
    // who wrote which slot, and when (state.hip: delta states): a stamp per slot, the capture epoch in an allocation of its own
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_slot_epoch, size_episodes * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetAsync(b->d_slot_epoch, 0, size_episodes * sizeof(uint32_t), ctx->stream);
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_epoch, sizeof(uint32_t));
    if (e == hipSuccess) e = hipMemsetD32Async((hipDeviceptr_t)b->d_epoch, (int)b->epoch, 1, ctx->stream);
    if (e != hipSuccess) {
        hp_set_error("hp_buffer_create: device allocation failed: %s", hipGetErrorString(e));
        hp_buffer_destroy(b);
        return HP_ERR_HIP;
    }
    *out = b;
    return HP_OK;
}

int hp_buffer_store(hp_buffer *b, hp_rng *rng, const double *obs, const double *ag, const double *g,
                    const double *actions, int64_t n_new) {
    HP_REQUIRE(b && rng && obs && ag && g && actions, HP_ERR_INVALID, "hp_buffer_store: null argument");
    HP_SERIALISE(b);
    HP_TRY(store_check(b, n_new, "hp_buffer_store"));
    return buffer_stage_and_store(b, rng, obs, ag, g, actions, n_new);
}

// ---- multi-process feeder support: episodes arrive in a host block the caller registered with the device
// (shared memory that worker processes write), laid out obs | ag | g | actions back to back like the library's own
// staging; the H2D copy reads it directly and asynchronously, the block may be rewritten once the returned ticket is done.
int hp_host_register(hp_ctx *ctx, void *host, size_t bytes) {
    HP_REQUIRE(ctx && host && bytes > 0, HP_ERR_INVALID, "hp_host_register: bad argument");
    CtxGuard guard(ctx);
    HP_CHECK_HIP(hipHostRegister(host, bytes, hipHostRegisterDefault));
    return HP_OK;
}

int hp_host_unregister(hp_ctx *ctx, void *host) {
    HP_REQUIRE(ctx && host, HP_ERR_INVALID, "hp_host_unregister: bad argument");
    CtxGuard guard(ctx);
    HP_CHECK_HIP(hipHostUnregister(host));
    return HP_OK;
}

int hp_buffer_store_pinned(hp_buffer *b, hp_rng *rng, const double *block, int64_t n_new, uint64_t *ticket) {
    HP_REQUIRE(b && rng && block, HP_ERR_INVALID, "hp_buffer_store_pinned: null argument");
    HP_SERIALISE(b);
    HP_TRY(store_check(b, n_new, "hp_buffer_store_pinned"));
    return buffer_stage_pinned(b, rng, block, n_new, ticket, true);
}

int hp_buffer_store_dev(hp_buffer *b, hp_rng *rng, const double *block_dev, int64_t n_new) {
    HP_REQUIRE(b && rng && block_dev, HP_ERR_INVALID, "hp_buffer_store_dev: null argument");
    HP_SERIALISE(b);
    HP_TRY(store_check(b, n_new, "hp_buffer_store_dev"));
    return buffer_stage_dev(b, rng, block_dev, n_new, true);
}

int hp_buffer_store_done(hp_buffer *b, uint64_t ticket, int32_t wait, int32_t *done) {
    HP_REQUIRE(b && done, HP_ERR_INVALID, "hp_buffer_store_done: null argument");
    hipEvent_t ev = nullptr;
    {
        HP_SERIALISE(b);
        HP_REQUIRE(ticket >= 1 && ticket <= b->pin_tickets, HP_ERR_INVALID, "hp_buffer_store_done: unknown ticket");
        if (ticket + hp_buffer::PIN_RING <= b->pin_tickets) {   // its event slot has been reused: that store is long done
            *done = 1;
            return HP_OK;
        }
        ev = b->pin_events[ticket % hp_buffer::PIN_RING];
    }
    // outside the context lock: a feeder waiting for its block must not stall the trainer's enqueues.  A concurrent
    // hp_buffer_store_pinned may re-record this very event object for ticket + PIN_RING in the meantime (it synchronises on
    // it first, so OUR copy is done by then): the slot is re-checked afterwards and a recycled slot reads as done, whatever
    // the wait / query observed of the newer copy
    hipError_t e = hipSuccess;
    if (wait) HP_CHECK_HIP(hipEventSynchronize(ev));
    else e = hipEventQuery(ev);
    if (e != hipSuccess && e != hipErrorNotReady) HP_CHECK_HIP(e);
    (void)hipGetLastError();
    *done = (e == hipSuccess) ? 1 : 0;
    if (!*done) {
        HP_SERIALISE(b);
        if (ticket + hp_buffer::PIN_RING <= b->pin_tickets) *done = 1;
    }
    return HP_OK;
}

int hp_buffer_stage(hp_buffer *b, const double *obs, const double *ag, const double *g, const double *actions,
                    int64_t n_new) {
    HP_REQUIRE(b && obs && ag && g && actions, HP_ERR_INVALID, "hp_buffer_stage: null argument");
    HP_SERIALISE(b);
    HP_REQUIRE(n_new > 0, HP_ERR_INVALID, "high <= 0");   // sample_her_transitions on an empty dict: randint(0, 0, T)
    return buffer_stage(b, obs, ag, g, actions, n_new);
}

int hp_buffer_info(hp_buffer *b, int64_t *size, int64_t *current_size, int64_t *n_transitions_stored, int32_t *T) {
    HP_REQUIRE(b, HP_ERR_INVALID, "hp_buffer_info: null handle");
    HP_SERIALISE(b);
    if (size) *size = b->size;
    if (current_size) *current_size = b->current_size;
    if (n_transitions_stored) *n_transitions_stored = b->n_transitions_stored;
    if (T) *T = b->T;
    return HP_OK;
}

int hp_buffer_debug_stage_info(hp_buffer *b, uint64_t *gen, uint64_t *ring_bytes, int32_t *ring_block) {
    HP_REQUIRE(b, HP_ERR_INVALID, "hp_buffer_debug_stage_info: null handle");
    HP_SERIALISE(b);
    if (gen) *gen = b->gen;
    if (ring_bytes) *ring_bytes = b->ring.bytes;
    if (ring_block) *ring_block = b->ring_cur;
    return HP_OK;
}

int hp_buffer_last_slots(hp_buffer *b, int64_t *host_out, int64_t n) {
    HP_REQUIRE(b && host_out, HP_ERR_INVALID, "hp_buffer_last_slots: null argument");
    HP_SERIALISE(b);
    HP_REQUIRE(n >= 0 && n <= b->staged_n, HP_ERR_INVALID, "hp_buffer_last_slots: n=%lld exceeds last store (%lld)",
               (long long)n, (long long)b->staged_n);
    HP_CHECK_HIP(hipMemcpyAsync(host_out, b->st_slots.p, n * 8, hipMemcpyDeviceToHost, b->ctx->stream));
    HP_CHECK_HIP(hipStreamSynchronize(b->ctx->stream));
    return HP_OK;
}

int hp_buffer_read(hp_buffer *b, int32_t which, int64_t first, int64_t n, double *host_out) {
    HP_REQUIRE(b && host_out, HP_ERR_INVALID, "hp_buffer_read: null argument");
    HP_SERIALISE(b);
    HP_REQUIRE(first >= 0 && n >= 0 && first + n <= b->size, HP_ERR_INVALID, "hp_buffer_read: range out of bounds");
    const double *src;
    size_t ep;
    switch (which) {
        case 0: src = b->d_obs; ep = b->ep_obs(); break;
        case 1: src = b->d_ag; ep = b->ep_ag(); break;
        case 2: src = b->d_g; ep = b->ep_g(); break;
        case 3: src = b->d_act; ep = b->ep_act(); break;
        default: hp_set_error("hp_buffer_read: which=%d not in 0..3", which); return HP_ERR_INVALID;
    }
    if (n == 0) return HP_OK;
    HP_CHECK_HIP(hipMemcpyAsync(host_out, src + first * ep, n * ep * 8, hipMemcpyDeviceToHost, b->ctx->stream));
    HP_CHECK_HIP(hipStreamSynchronize(b->ctx->stream));
    return HP_OK;
}

// Throughput mode (storage_dtype = fp32): builds the float32 mirror of observations and actions (+ the packed float64
// goals) from what the buffer holds and keeps it current behind every later store; hp_buffer_sample_dev_f32 (sampler.hip) reads it.
int hp_buffer_enable_f32_rows(hp_buffer *b) {
    HP_REQUIRE(b, HP_ERR_INVALID, "hp_buffer_enable_f32_rows: null handle");
    HP_SERIALISE(b);
    if (b->p_row) return HP_OK;
    const int row_w = (b->obs_dim + b->act_dim + 31) / 32 * 32, goal_w = (2 * b->goal_dim + 7) / 8 * 8;
    HP_REQUIRE(row_w == 32 && b->obs_dim <= 28 && b->goal_dim <= 4, HP_ERR_INVALID,
               "hp_buffer_enable_f32_rows: needs obs_dim <= 28, obs_dim + act_dim <= 32 (one 128-byte line of float32 per timestep) and "
               "goal_dim <= 4; got %d, %d, %d", b->obs_dim, b->act_dim, b->goal_dim);
    const size_t rows = (size_t)b->size * (b->T + 1);
    HP_CHECK_HIP(hipMalloc((void **)&b->p_row, rows * row_w * sizeof(float)));
    if (hipMalloc((void **)&b->p_goal, rows * goal_w * sizeof(double)) != hipSuccess) {
        (void)hipFree(b->p_row);
        b->p_row = nullptr;
        hp_set_error("hp_buffer_enable_f32_rows: cannot allocate the goal rows");
        return HP_ERR_HIP;
    }
    b->row_w = row_w;
    b->goal_w = goal_w;
    ++b->gen;   // a cycle captured before now does not refresh the rows
    return launch_pack(b, nullptr, 0, b->size);      // (rows of unfilled slots hold whatever the allocation held: never sampled)
}

// ---- compute_reward / _is_success (bmirobot_env_push_F.py:84-90, :243-245) as batched device ops ------------------
static int goal_reward_launch(hp_ctx *ctx, const double *ag, const double *g, int64_t n, int32_t goal_dim, double thr_sq,
                              int mode, float *out32, double *out64) {
    hipLaunchKernelGGL(k_goal_reward, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, ag, g, (long long)n,
                       (int)goal_dim, thr_sq, mode, out32, out64);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// smallest double s whose correctly rounded square root is > thr (strict) or >= thr: the predicates d > thr and
// !(d < thr) in the squared domain (sqrt_rn is monotone), so no device square root and no rounding mismatch
extern "C++" double squared_bound(double thr, bool strict) {   // internal.h: episode_stats.hip takes its thresholds from here too
    if (!(thr >= 0.0)) return 0.0;
    double s = thr * thr;
    auto hit = [&](double v) { const double r = std::sqrt(v); return strict ? r > thr : r >= thr; };
    while (s > 0.0 && hit(s)) s = std::nextafter(s, -INFINITY);
    while (!hit(s)) s = std::nextafter(s, INFINITY);
    return s;
}

int hp_compute_reward_dev(hp_ctx *ctx, const double *ag_dev, const double *g_dev, int64_t n, int32_t goal_dim,
                          double distance_threshold, int32_t dense, float *sparse_out_dev, double *dense_out_dev) {
    HP_REQUIRE(ctx && ag_dev && g_dev, HP_ERR_INVALID, "hp_compute_reward_dev: null argument");
    CtxGuard guard(ctx);
    HP_REQUIRE(n >= 0 && goal_dim > 0, HP_ERR_INVALID, "hp_compute_reward_dev: bad shape");
    HP_REQUIRE(dense ? dense_out_dev != nullptr : sparse_out_dev != nullptr, HP_ERR_INVALID,
               "hp_compute_reward_dev: the output of the selected reward type is null");
    if (n == 0) return HP_OK;
    return goal_reward_launch(ctx, ag_dev, g_dev, n, goal_dim, dense ? 0.0 : squared_bound(distance_threshold, true),
                              dense ? 1 : 0, sparse_out_dev, dense_out_dev);
}

int hp_is_success_dev(hp_ctx *ctx, const double *ag_dev, const double *g_dev, int64_t n, int32_t goal_dim,
                      double distance_threshold, float *out_dev) {
    HP_REQUIRE(ctx && ag_dev && g_dev && out_dev, HP_ERR_INVALID, "hp_is_success_dev: null argument");
    CtxGuard guard(ctx);
    HP_REQUIRE(n >= 0 && goal_dim > 0, HP_ERR_INVALID, "hp_is_success_dev: bad shape");
    if (n == 0) return HP_OK;
    return goal_reward_launch(ctx, ag_dev, g_dev, n, goal_dim, squared_bound(distance_threshold, false), 2, out_dev,
                              nullptr);
}

// host-array forms (the GoalEnv API hands numpy arrays over): staged through the device, same kernels
static int goal_reward_host(hp_ctx *ctx, const double *ag, const double *g, int64_t n, int32_t goal_dim, double thr_sq,
                            int mode, void *out_host) {
    DevBuf &ws = ctx->reward_ws;     // guarded by the context lock the callers hold
    const size_t nb = (size_t)n * goal_dim * 8, ob = (size_t)n * (mode == 1 ? 8 : 4);
    HP_TRY(ws.ensure(2 * nb + ob));
    char *d = ws.as<char>();
    hipStream_t s = ctx->stream;
    HP_CHECK_HIP(hipMemcpyAsync(d, ag, nb, hipMemcpyHostToDevice, s));
    HP_CHECK_HIP(hipMemcpyAsync(d + nb, g, nb, hipMemcpyHostToDevice, s));
    HP_TRY(goal_reward_launch(ctx, reinterpret_cast<double *>(d), reinterpret_cast<double *>(d + nb), n, goal_dim, thr_sq,
                              mode, reinterpret_cast<float *>(d + 2 * nb), reinterpret_cast<double *>(d + 2 * nb)));
    HP_CHECK_HIP(hipMemcpyAsync(out_host, d + 2 * nb, ob, hipMemcpyDeviceToHost, s));
    HP_CHECK_HIP(hipStreamSynchronize(s));
    return HP_OK;
}

int hp_compute_reward(hp_ctx *ctx, const double *ag_host, const double *g_host, int64_t n, int32_t goal_dim,
                      double distance_threshold, int32_t dense, float *sparse_out_host, double *dense_out_host) {
    HP_REQUIRE(ctx && ag_host && g_host, HP_ERR_INVALID, "hp_compute_reward: null argument");
    CtxGuard guard(ctx);
    HP_REQUIRE(n >= 0 && goal_dim > 0, HP_ERR_INVALID, "hp_compute_reward: bad shape");
    HP_REQUIRE(dense ? dense_out_host != nullptr : sparse_out_host != nullptr, HP_ERR_INVALID,
               "hp_compute_reward: the output of the selected reward type is null");
    if (n == 0) return HP_OK;
    return goal_reward_host(ctx, ag_host, g_host, n, goal_dim, dense ? 0.0 : squared_bound(distance_threshold, true),
                            dense ? 1 : 0, dense ? (void *)dense_out_host : (void *)sparse_out_host);
}

int hp_is_success(hp_ctx *ctx, const double *ag_host, const double *g_host, int64_t n, int32_t goal_dim,
                  double distance_threshold, float *out_host) {
    HP_REQUIRE(ctx && ag_host && g_host && out_host, HP_ERR_INVALID, "hp_is_success: null argument");
    CtxGuard guard(ctx);
    HP_REQUIRE(n >= 0 && goal_dim > 0, HP_ERR_INVALID, "hp_is_success: bad shape");
    if (n == 0) return HP_OK;
    return goal_reward_host(ctx, ag_host, g_host, n, goal_dim, squared_bound(distance_threshold, false), 2, out_host);
}

void hp_buffer_destroy(hp_buffer *b) {
    if (!b) return;
    if (b->d_obs) (void)hipFree(b->d_obs);
    if (b->d_ag) (void)hipFree(b->d_ag);
    if (b->d_g) (void)hipFree(b->d_g);
    if (b->d_act) (void)hipFree(b->d_act);
    if (b->d_meta) (void)hipFree(b->d_meta);
    if (b->d_slot_epoch) (void)hipFree(b->d_slot_epoch);
    if (b->d_epoch) (void)hipFree(b->d_epoch);
    b->dirty_counts.release();
    if (b->p_row) (void)hipFree(b->p_row);
    if (b->p_goal) (void)hipFree(b->p_goal);
    for (hipEvent_t ev : b->pin_events)
        if (ev) (void)hipEventDestroy(ev);
    b->st_obs.release();
    b->st_slots.release();
    b->pin.release();
    {
        HipStageApi api;
        b->ring.release(api);
    }
    b->plan.release();
    b->out.release();
    delete b;
}

}  // extern "C"
