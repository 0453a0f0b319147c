// internal.h -- shared declarations of librlarm_hip.so (not part of the C ABI).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "rlarm_hip.h"
#include "rlarm_hip_debug.h"
#include "stage_ring.h"

// ------------------------------------------------------------------ error plumbing
void hp_set_error(const char *fmt, ...);

// launch log (hp_agent_update_kernels, rlarm_hip_debug.h): while non-null on the calling thread, every launch site on the path of
// an update sequence records the kernel it enqueues -- the names bench.py reports are read off the launch logic itself
extern thread_local std::vector<std::string> *hp_klog;
#define HP_KLOG(name) do { if (hp_klog) hp_klog->push_back(name); } while (0)

#define HP_CHECK_HIP(expr)                                                                   \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess) {                                                              \
            hp_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return HP_ERR_HIP;                                                               \
        }                                                                                    \
    } while (0)

#define HP_REQUIRE(cond, code, ...)   \
    do {                              \
        if (!(cond)) {                \
            hp_set_error(__VA_ARGS__); \
            return (code);            \
        }                             \
    } while (0)

#define HP_TRY(expr)              \
    do {                          \
        int _s = (expr);          \
        if (_s != HP_OK) return _s; \
    } while (0)

// small RAII-less device buffer helper (grow-only)
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return HP_OK;
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        HP_CHECK_HIP(hipMalloc(&p, need));
        bytes = need;
        return HP_OK;
    }
    void release() {
        if (p) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// ------------------------------------------------------------------ stream capture
struct GraphExec {   // an instantiated hipGraph, destroyed with its owner
    hipGraphExec_t h = nullptr;
    GraphExec() = default;
    GraphExec(GraphExec &&o) noexcept : h(o.h) { o.h = nullptr; }
    GraphExec &operator=(GraphExec &&o) noexcept { std::swap(h, o.h); return *this; }
    ~GraphExec() { if (h) (void)hipGraphExecDestroy(h); }
};
struct Captured {
    int st = HP_OK;              // what the enqueueing callable returned: the launch logic failed
    hipError_t e = hipSuccess;   // the runtime refused the capture or its instantiation
    GraphExec exec;              // set when both succeeded and the capture was not a dry run
    int status() const {         // HP_OK or the first failure, with the error message set
        if (st != HP_OK) return st;
        HP_REQUIRE(e == hipSuccess, HP_ERR_HIP, "stream capture failed: %s", hipGetErrorString(e));
        return HP_OK;
    }
};
// Records what enqueue() puts on s under a thread-local capture and instantiates it -- or discards it (instantiate = false: a dry
// run).  Nothing enqueued runs here.  The hipGraph_t is destroyed on every path; a runtime error is cleared from HIP's last error.
template <class F> Captured capture_graph(hipStream_t s, F &&enqueue, bool instantiate = true) {
    Captured c;
    c.e = hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal);
    if (c.e == hipSuccess) {
        c.st = enqueue();
        hipGraph_t g = nullptr;
        c.e = hipStreamEndCapture(s, &g);
        if (c.st == HP_OK && c.e == hipSuccess && instantiate) c.e = hipGraphInstantiate(&c.exec.h, g, nullptr, nullptr, 0);
        if (g) (void)hipGraphDestroy(g);
    }
    if (c.e != hipSuccess) {
        c.exec.h = nullptr;
        (void)hipGetLastError();
    }
    return c;
}

// ------------------------------------------------------------------ context
struct hp_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // stream kernels are enqueued on
    hipStream_t own_stream = nullptr;  // created by the context
    hipEvent_t order_ev = nullptr;     // hp_ctx_set_stream: orders the new stream behind the old one's work
    // hp_ctx_borrow_stream / hp_ctx_return_stream (context.hip): the stream to go back to while a caller's stream is borrowed; a
    // borrowed stream whose work the own stream has not been ordered behind yet; has the own stream been used since the last borrow?
    hipStream_t borrowed_from = nullptr, foreign = nullptr;
    bool own_dirty = true;
    hipEvent_t fence_ev[2] = {nullptr, nullptr};   // own -> borrowed, borrowed -> own
    int cu_count = 0;
    char name[128] = {0};
    // Every entry point that enqueues on the stream or touches a handle's host mirror holds this for the duration of the
    // call: the counterpart of the reference's per-object locks (replay_buffer.py:29,34,48; normalizer.py:22,27,42), so a
    // host feeder thread may call hp_buffer_store while another thread drives hp_agent_train_cycle.  Recursive because
    // entry points call each other.
    std::recursive_mutex mu;
    DevBuf reward_ws;                  // scratch of the host-array forms of hp_compute_reward / hp_is_success
};
void ctx_join_foreign(hp_ctx *c);   // context.hip: order the context's stream behind the work of a stream that was borrowed
struct CtxGuard {   // + the calling thread's current device: HIP keeps that per thread and a feeder thread starts on device 0
    std::lock_guard<std::recursive_mutex> g;
    explicit CtxGuard(hp_ctx *c) : g(c->mu) {
        (void)hipSetDevice(c->device);
        if (!c->borrowed_from) {         // (inside a borrow the launches go to the caller's stream: nothing to join, nothing dirtied)
            if (c->foreign) ctx_join_foreign(c);
            c->own_dirty = true;
        }
    }
};
#define HP_SERIALISE(handle) CtxGuard hp_serialise_guard_((handle)->ctx)

// pinned host staging for async H2D copies of caller-owned (pageable) arrays: the caller's memory
// is only touched by a CPU memcpy during the call; `fence` marks the last DMA that read the buffer.
struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    hipEvent_t fence = nullptr;
    bool pending = false;
    int ensure(size_t need) {
        if (!fence) HP_CHECK_HIP(hipEventCreateWithFlags(&fence, hipEventDisableTiming));
        if (pending) {
            HP_CHECK_HIP(hipEventSynchronize(fence));
            pending = false;
        }
        if (need <= bytes) return HP_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
        HP_CHECK_HIP(hipHostMalloc(&p, need, hipHostMallocDefault));
        bytes = need;
        return HP_OK;
    }
    int mark(hipStream_t s) {
        HP_CHECK_HIP(hipEventRecord(fence, s));
        pending = true;
        return HP_OK;
    }
    void release() {
        if (pending && fence) (void)hipEventSynchronize(fence);
        if (p) (void)hipHostFree(p);
        if (fence) (void)hipEventDestroy(fence);
        p = nullptr;
        fence = nullptr;
        bytes = 0;
        pending = false;
    }
};

// The HIP side of StageRing (stage_ring.h): blocks the device reads in place through their mapped address.
struct HipStageApi {
    using Event = hipEvent_t;
    using Stream = hipStream_t;
    int alloc(size_t bytes, void **host, void **dev) {
        *host = *dev = nullptr;
        HP_CHECK_HIP(hipHostMalloc(host, bytes, hipHostMallocMapped | hipHostMallocCoherent));
        HP_CHECK_HIP(hipHostGetDevicePointer(dev, *host, 0));
        return HP_OK;
    }
    void free_block(void *host) { (void)hipHostFree(host); }
    int event_create(Event *e) {
        HP_CHECK_HIP(hipEventCreateWithFlags(e, hipEventDisableTiming));
        return HP_OK;
    }
    int event_sync(Event e) {
        HP_CHECK_HIP(hipEventSynchronize(e));
        return HP_OK;
    }
    int event_record(Event e, Stream s) {
        HP_CHECK_HIP(hipEventRecord(e, s));
        return HP_OK;
    }
    void event_destroy(Event e) { (void)hipEventDestroy(e); }
};

// ------------------------------------------------------------------ random stream
#define MT_N 624
struct MtState {  // device-resident, same fields as numpy's legacy state tuple
    uint32_t key[MT_N];
    int32_t pos;
    int32_t has_gauss;   // legacy_gauss's cached second normal (numpy's has_gauss / gauss): written by the normal draws only
    double gauss;
};
static_assert(sizeof(MtState) == MT_N * 4 + 16, "MtState: key | pos | has_gauss | gauss");

// numpy _legacy_seeding(int) -> mt19937_seed() -> init_genrand: the key of RandomState(seed) (its pos is 624, no cached normal)
__host__ __device__ inline void mt_init_genrand(uint32_t seed, uint32_t *key) {
    for (uint32_t i = 0; i < MT_N; ++i) {
        key[i] = seed;
        seed = 1812433253u * (seed ^ (seed >> 30)) + i + 1u;
    }
}

// n whole legacy states side by side in one allocation.  As hp_rng_streams: one exploration stream per environment of a
// vectorised simulator (rng_streams.hip, k_rollout_step_streams in rollout.hip), stream i belonging to row i of a rollout wave.
struct hp_rng_streams {
    hp_ctx *ctx = nullptr;
    int64_t n = 1;
    MtState *d_state = nullptr;   // [n]
};
// The host round trip of MtStates (rng_streams.hip): `count` states between `host` and d_state + first, on the context's stream,
// waited for (the host side is pageable).  mt_state_fill makes one state from the fields of numpy's state tuple: the one place
// that checks pos and drops a cached normal that is not given (`stream` < 0: the message does not name a stream).
int mt_states_get(hp_rng_streams *s, MtState *host, int64_t first, int64_t count);
int mt_states_put(hp_rng_streams *s, const MtState *host, int64_t first, int64_t count);
int mt_state_fill(MtState &h, const char *entry, int64_t stream, const uint32_t *key624, int32_t pos, int32_t has_gauss, double gauss);

struct hp_rng : hp_rng_streams {   // the one stream of the sampler: n = 1
    DevBuf scratch;  // test-hook outputs
    // parallel form of the sampler's index draw + hp_rng_advance (rng_parallel.hip)
    int64_t par_min_batch = 0;       // hp_rng_set_parallel: draws of at least this many transitions take it; 0 = off
    int64_t par_debug_window = 0;    // hp_rng_debug_set_window: stream words the NEXT parallel draw may use (0 = all it sized)
    struct ParCtl *d_par = nullptr;  // device: cursors between the passes, commit / fall-back flags, counters
    DevBuf par_raw, par_win, par_counts, par_table, par_poly;   // raw stream, 33-block window, chunk counts, jump polynomials
    std::vector<uint64_t> par_polys; // host copy of the segment table: g_{p S}, p = 1 .. size / 312
    double par_table_ms = 0;         // host time spent building it (reported once in DESIGN 3.6)
};
void rng_parallel_release(hp_rng *rng);

// one drawn transition index record (her.py:24-33)
struct __attribute__((aligned(16))) PlanRec {
    int32_t e;    // episode index
    int32_t t;    // timestep
    int32_t fut;  // t + 1 + int(u2 * (T - t))
    int32_t her;  // u1 < future_p
};

// ------------------------------------------------------------------ replay buffer
struct BufMeta {  // device-resident mirror of replay_buffer's counters
    int64_t current_size;
    int64_t n_transitions_stored;
};

struct hp_buffer {
    hp_ctx *ctx = nullptr;
    int64_t size = 0;  // capacity in episodes
    int32_t T = 0, obs_dim = 0, goal_dim = 0, act_dim = 0;
    double *d_obs = nullptr, *d_ag = nullptr, *d_g = nullptr, *d_act = nullptr;
    BufMeta *d_meta = nullptr;
    // Delta states (state.hip).  slot_epoch[slot] = the value of *d_epoch when the slot was last scattered into (0: never, or not
    // since the last restore); every capture records *d_epoch and then advances it, so a slot is dirty with respect to a capture c
    // iff its stamp is > c.  The scatter kernels read *d_epoch at run time (store_device.h).  epoch mirrors *d_epoch (only captures
    // and restores move it, all enqueued by the host); stamps older than min_since were zeroed by a restore.
    uint32_t *d_slot_epoch = nullptr, *d_epoch = nullptr;
    uint32_t epoch = 1, min_since = 0;
    DevBuf dirty_counts;   // per-chunk counts of the dirty scan
    // host mirror (slot policy is deterministic given n_new, so the host can track it)
    int64_t current_size = 0, n_transitions_stored = 0;
    // staging of the most recent store_episode batch (also the source of _update_normalizer)
    // one allocation (st_obs) holds obs | ag | g | actions of the staged batch, so the upload is ONE copy
    DevBuf st_obs, st_slots;
    double *st_ag = nullptr, *st_g = nullptr, *st_act = nullptr;
    PinnedBuf pin;                     // eager stores, and the cycle path in its copy form (RLARM_CYCLE_OPEN=copy)
    // hp_agent_train_cycle, opening launch on: the fresh episodes stay in a pinned block of this ring, in the same
    // obs | ag | g | actions layout, and k_cycle_open reads them there (no H2D copy); it fills st_obs .. st_act itself.
    // ring_cur: the block of the cycle being enqueued, -1 = the staging was (or will be) filled by a copy.
    StageRing<HipStageApi> ring;
    int ring_cur = -1;
    int64_t staged_n = 0;
    // hp_buffer_store_pinned: tickets of the asynchronous copies out of caller-registered host blocks
    static constexpr int PIN_RING = 16;
    hipEvent_t pin_events[PIN_RING] = {nullptr};
    uint64_t pin_tickets = 0;
    // Throughput rows (hp_buffer_enable_f32_rows; SURVEY 8b `storage_dtype`): a float32 mirror of observations + actions packed one
    // (episode, timestep) per 128-byte line, and the goals (kept float64: rewards and relabelled goals stay bit-exact) packed
    // [ag_t | g_t] per 64-byte half line -- what hp_buffer_sample_dev_f32 reads.  Maintained behind every scatter.
    float *p_row = nullptr;      // [size][T + 1][row_w] floats: obs_t | actions_t (zeros at t = T) | 0
    double *p_goal = nullptr;    // [size][T + 1][goal_w] doubles: ag_t | g_t (zeros at t = T) | 0
    int32_t row_w = 0, goal_w = 0;
    // sampling scratch
    DevBuf plan, out;
    uint64_t gen = 0;   // bumped whenever what a captured cycle reads moves or appears (staging reallocated, throughput rows enabled)
    size_t ep_obs() const { return (size_t)(T + 1) * obs_dim; }
    size_t ep_ag() const { return (size_t)(T + 1) * goal_dim; }
    size_t ep_g() const { return (size_t)T * goal_dim; }
    size_t ep_act() const { return (size_t)T * act_dim; }
};
int buffer_launch_pack(hp_buffer *b, int64_t n_new);   // refresh the throughput rows of the episodes just scattered (no-op when off)
int buffer_launch_pack_range(hp_buffer *b, int64_t first, int64_t n);   // ... of episodes [first, first + n) (hp_state_restore)

// ------------------------------------------------------------------ normalizer
#define NORM_MAX 256   // columns a normalizer can hold (bmirobot: 27 observations, 3 goals); hp_norm_create rejects more
struct NormDev {  // device-resident state; size <= NORM_MAX columns
    float local_sum[NORM_MAX], local_sumsq[NORM_MAX], local_count[4];
    float total_sum[NORM_MAX], total_sumsq[NORM_MAX], total_count[4];
    float sync[2 * NORM_MAX + 4];  // sum | sumsq | count snapshot exchanged between ranks
    float mean[NORM_MAX];
    double std[NORM_MAX];  // float64-valued (std_f32: float32 value widened)
};

struct hp_norm {
    hp_ctx *ctx = nullptr;
    int32_t size = 0;
    double eps = 1e-2, clip = 0;
    int32_t std_f32 = 0;
    NormDev *d = nullptr;
    DevBuf scratch, scratch2;
    PinnedBuf pin;
    bool in_recompute = false;
};

// ------------------------------------------------------------------ rollout block
// A block of n episodes in the staging layout (rollout.hip); episode_stats.hip reads its ag and g arrays in place.
struct hp_rollout {
    hp_ctx *ctx = nullptr;
    int64_t n = 0;                 // episodes the block holds
    int32_t T = 0, od = 0, gd = 0, ad = 0;
    int64_t first = 0, rows = 0;   // the wave being collected: episodes [first, first + rows)
    double action_max = 1.0;       // of the policy whose outputs a teacher-forced step is handed (hp_rollout_set_action_max)
    int64_t launch_cap = HP_ROLLOUT_MAX_LAUNCH_TIMESTEPS;   // timesteps (waves x T) one launch of hp_rollout_waves may hold
    double *block = nullptr;
    int64_t o_ag = 0, o_g = 0, o_act = 0, elems = 0;   // offsets in float64 elements (feeder._Layout)
};

// the block's four arrays at episode `episode`, into an argument block that names them b_obs / b_ag / b_g / b_act
template <class Args>
inline void rollout_arrays_at(const hp_rollout *ro, int64_t episode, Args &A) {
    A.b_obs = ro->block + episode * (ro->T + 1) * ro->od;
    A.b_ag = ro->block + ro->o_ag + episode * (ro->T + 1) * ro->gd;
    A.b_g = ro->block + ro->o_g + episode * ro->T * ro->gd;
    A.b_act = ro->block + ro->o_act + episode * ro->T * ro->ad;
}

// smallest double s whose correctly rounded square root is > thr (strict) or >= thr (buffer.hip): the predicates d > thr and
// !(d < thr) of compute_reward / _is_success in the squared domain (the device side: hp_reward, transition_device.h)
double squared_bound(double thr, bool strict);

// rank exchange (comm.hip): one RCCL communicator bound to the context's stream
struct hp_comm {
    hp_ctx *ctx = nullptr;
    void *nccl = nullptr;   // ncclComm_t
    int rank = 0, world = 1;
};
int comm_allreduce_sum_f32(hp_comm *c, float *dev, size_t n);    // utils.py:43-48
int comm_allreduce_mean_f32(hp_comm *c, float *dev, size_t n);   // normalizer.py:60-64

// launchers implemented in the .hip files -------------------------------------------------
// rng.hip
int rng_launch_plan(hp_rng *rng, const BufMeta *d_meta, int64_t n_eps_fixed, int32_t T, int64_t batch,
                    int32_t n_batches, double future_p, PlanRec *d_plan, hipStream_t stream = nullptr);
int rng_launch_slots(hp_rng *rng, hp_buffer *buf, int64_t n_new, int64_t *d_slots);
// rng_parallel.hip: the index draw of the three sampler entry points -- rng_launch_plan, or its parallel form behind
// hp_rng_set_parallel (same words, same plan, same final state)
int rng_launch_plan_sample(hp_rng *rng, const BufMeta *d_meta, int32_t T, int64_t batch, double future_p, PlanRec *d_plan);
// normalizer plan (batch_first transitions out of n_first staged episodes) + the first n_batches minibatch plans, one launch
int rng_launch_plan2(hp_rng *rng, int64_t n_first, int32_t T, int64_t batch_first, PlanRec *d_plan_first,
                     const BufMeta *d_meta, int64_t batch, int32_t n_batches, double future_p, PlanRec *d_plan);

// sampler.hip
int buffer_launch_gather_dict(hp_buffer *buf, const PlanRec *d_plan, int64_t batch, double sq_threshold,
                              double *d_out, float *d_r, double *d_r64);
// buffer.hip
int buffer_stage_and_store(hp_buffer *b, hp_rng *rng, const double *obs, const double *ag, const double *g,
                           const double *actions, int64_t n_new);
// the staging half alone (+ the host mirror of the counters): slots and scatter follow in k_cycle_open (cycle_open.hip).
// direct: the episodes go into the next block of b->ring and no further (k_cycle_open reads them there; the caller marks the block
// behind that launch, buffer_mark_cycle_block); otherwise pinned copy + H2D into the device staging
int buffer_stage_for_cycle(hp_buffer *b, const double *obs, const double *ag, const double *g, const double *actions,
                           int64_t n_new, bool direct);
int buffer_mark_cycle_block(hp_buffer *b);
// the same out of a device-registered host block (feeder ring); store_now: slots + scatter follow at once
int buffer_stage_pinned(hp_buffer *b, hp_rng *rng, const double *block, int64_t n_new, uint64_t *ticket, bool store_now);
// the same out of a DEVICE block (a rollout wave collected on the device, rollout.hip): a device-to-device copy, no ticket
int buffer_stage_dev(hp_buffer *b, hp_rng *rng, const double *block_dev, int64_t n_new, bool store_now);

// agent_engines.hip: the one launch of k_policy_slab8 (slab8.h), a workgroup per 4 rows of P
struct PolicyArgs;
int launch_policy_slab(hipStream_t stream, const PolicyArgs &P);
// agent_forward.hip: hp_agent_act on device rows, actions left on the device, nothing copied, no host wait
int agent_act_dev(hp_agent *a, hp_norm *on, hp_norm *gn, int32_t net, const double *obs_dev, const double *g_dev, int64_t rows,
                  double clip_obs, float *actions_dev);

// norm.hip
int norm_launch_update_from_plan(hp_norm *o, hp_norm *g, hp_buffer *b, const PlanRec *d_plan, int64_t rows,
                                 double clip_obs, bool recompute);
int norm_launch_begin(hp_norm *nz);
int norm_launch_end(hp_norm *nz);
