// state.hip -- the training state: everything a continued run needs (both networks and their targets, Adam m / v / step, both
// normalizers, the MT19937 stream, the replay buffer's episodes and counters) captured into a snapshot arena in stream order,
// drained to pinned host memory on a second stream, and restored -- after a device-side checksum of what was uploaded -- into live
// objects.  The reference has the wish only (ddpg_agent.py:54-62, "load the data to continue the training", commented out).
//   capture   ctx stream: k_state_flat (arena -> flat order, 8 vectors) | k_state_small | 4 device-to-device row copies | event
//             drain stream: wait(event) | k_checksum per section | chunked copies to pinned memory | event
//   restore   upload into the SAME arena | k_checksum per section, compared with the caller's sums | only then: k_state_flat /
//             k_state_small / row copies the other way, relayout of both parameter sets, throughput rows, host mirrors
//   delta     as capture, with the buffer captured as the slots stamped since a base capture: k_dirty_count | k_dirty_scan |
//             k_dirty_emit (ascending slot list) | k_delta_pack (their rows) instead of the four whole-array copies
#include "state.h"

typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
typedef double f64x2 __attribute__((ext_vector_type(2)));

#define ST_ALIGN 256                    // section offsets in the blob
#define ST_DRAIN_CHUNK (16u << 20)      // bytes per copy of the drain

struct StateArena {
    char *dev = nullptr;          // the snapshot (capture) / the uploaded state (restore)
    size_t dev_bytes = 0;
    u64 *d_sums = nullptr;        // 2 * DS_SECTIONS: (A, B) per section (a full state uses the first 2 * ST_SECTIONS)
    char *pin = nullptr;          // pinned host copy of the snapshot, filled by the drain
    size_t pin_bytes = 0;
    u64 *pin_sums = nullptr;
    hipStream_t drain = nullptr;
    hipEvent_t captured = nullptr, drained = nullptr;
    uint64_t ticket = 0;          // of the most recent capture
    bool pending = false;         // ... which has not been fetched (or abandoned) yet
    size_t bytes = 0;             // ... and its blob size
    bool delta = false;           // ... and its kind: a full state (ST_SECTIONS sections) or a delta (DS_SECTIONS)
    size_t hdr_off = 0;           // ... a delta's header section in the blob
    uint32_t capture_epoch = 0;   // the buffer epoch the most recent capture recorded (host mirror)
};

// ------------------------------------------------------------------------------- kernels
// Position-weighted checksum of a section read as little-endian 64-bit words w_0 .. w_{n-1} (the last one zero-padded):
// A = sum w_i, B = sum (i + 1) w_i, both mod 2^64.  Both sums are associative and commutative, so the grid shape does not
// matter: grid-stride over 16-byte loads (four in flight per lane), wave reduction, one pair of 64-bit atomic adds per
// workgroup.  The words that do not fit the 16-byte body (a leading one when the section starts 8 mod 16, a trailing odd one,
// the padded tail) are added by one thread.
__device__ __forceinline__ void sum_pair(const u64x2 x, u64 i0, u64 &a, u64 &b) {
    a += x.x + x.y;
    b += (i0 + 1ull) * x.x + (i0 + 2ull) * x.y;
}

__device__ __forceinline__ void checksum_body(const u64 *__restrict__ w, u64 nwords, unsigned tail_bytes, u64 *out) {
    const u64 head = (nwords > 0 && ((uintptr_t)w & 8u)) ? 1ull : 0ull;
    const u64x2 *v = reinterpret_cast<const u64x2 *>(w + head);
    const u64 npairs = (nwords - head) / 2;
    const u64 stride = (u64)gridDim.x * blockDim.x;
    u64 p = (u64)blockIdx.x * blockDim.x + threadIdx.x;
    u64 a = 0, b = 0;
    for (; p + 3 * stride < npairs; p += 4 * stride) {
        const u64x2 x0 = __builtin_nontemporal_load(v + p), x1 = __builtin_nontemporal_load(v + p + stride),
                    x2 = __builtin_nontemporal_load(v + p + 2 * stride), x3 = __builtin_nontemporal_load(v + p + 3 * stride);
        sum_pair(x0, head + 2 * p, a, b);
        sum_pair(x1, head + 2 * (p + stride), a, b);
        sum_pair(x2, head + 2 * (p + 2 * stride), a, b);
        sum_pair(x3, head + 2 * (p + 3 * stride), a, b);
    }
    for (; p < npairs; p += stride) sum_pair(__builtin_nontemporal_load(v + p), head + 2 * p, a, b);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (head) { a += w[0]; b += w[0]; }
        if ((nwords - head) & 1ull) { a += w[nwords - 1]; b += nwords * w[nwords - 1]; }
        if (tail_bytes) {
            const unsigned char *t = reinterpret_cast<const unsigned char *>(w + nwords);
            u64 x = 0;
            for (unsigned k = 0; k < tail_bytes; ++k) x |= (u64)t[k] << (8 * k);
            a += x;
            b += (nwords + 1ull) * x;
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_down(a, off);
        b += __shfl_down(b, off);
    }
    __shared__ u64 red[2][4];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { red[0][wave] = a; red[1][wave] = b; }
    __syncthreads();
    if (threadIdx.x == 0) {
        a = red[0][0] + red[0][1] + red[0][2] + red[0][3];
        b = red[1][0] + red[1][1] + red[1][2] + red[1][3];
        if (a) atomicAdd(out, a);
        if (b) atomicAdd(out + 1, b);
    }
}

__global__ __launch_bounds__(256) void k_checksum(const u64 *__restrict__ w, u64 nwords, unsigned tail_bytes, u64 *out) {
    checksum_body(w, nwords, tail_bytes, out);
}

// the used prefix of a delta's slot list or packed rows: hdr[0] episodes (never more than the section has room for)
__global__ __launch_bounds__(256) void k_checksum_prefix(const u64 *__restrict__ w, const long long *__restrict__ hdr,
                                                         u64 words_per_ep, long long max_dirty, u64 *out) {
    const long long n = hdr[0] < max_dirty ? hdr[0] : max_dirty;
    checksum_body(w, (u64)n * words_per_ep, 0u, out);
}

// eight parameter-shaped vectors between the padded arena and the reference's flat order: blockIdx.y = vector
struct FlatArgs {
    float *arena[8];   // live arenas: params, params, targets, targets, adam_m, adam_v, adam_m, adam_v
    float *flat[8];    // sections ST_ACTOR .. ST_ADAM_CRITIC_V of the snapshot
    FlatMap m[2];      // actor, critic
};

template <bool RESTORE> __global__ __launch_bounds__(256) void k_state_flat(const FlatArgs A) {
    const int vec = blockIdx.y;
    const FlatMap &m = A.m[(vec == 1 || vec == 3 || vec >= 6) ? 1 : 0];   // actor | critic
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= m.n) return;
    const int i = flat_to_arena(m, j);
    if (RESTORE) A.arena[vec][i] = A.flat[vec][j];   // the arena's padding is zero and stays zero (agent.h)
    else A.flat[vec][j] = A.arena[vec][i];
}

// the small state: both normalizers (every field of NormDev but the `sync` scratch), the MT19937 key and position, the Adam
// step, the buffer's counters.  One workgroup.
struct SmallArgs {
    NormDev *nz[2];
    int size[2];
    MtState *rng;
    AgentDevState *st;
    BufMeta *meta;
    char *base;
    long long off[ST_SECTIONS];
};

template <bool RESTORE, class T> __device__ __forceinline__ void small_copy(T *live, T *snap, int n) {
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        if (RESTORE) live[i] = snap[i];
        else snap[i] = live[i];
    }
}

template <bool RESTORE> __global__ __launch_bounds__(256) void k_state_small(const SmallArgs A) {
    for (int k = 0; k < 2; ++k) {
        NormDev *nz = A.nz[k];
        const int s0 = k ? ST_GNORM : ST_ONORM, n = A.size[k];
        auto f32 = [&](int f) { return reinterpret_cast<float *>(A.base + A.off[s0 + f]); };
        small_copy<RESTORE>(nz->local_sum, f32(NF_LOCAL_SUM), n);
        small_copy<RESTORE>(nz->local_sumsq, f32(NF_LOCAL_SUMSQ), n);
        small_copy<RESTORE>(nz->local_count, f32(NF_LOCAL_COUNT), 1);
        small_copy<RESTORE>(nz->total_sum, f32(NF_TOTAL_SUM), n);
        small_copy<RESTORE>(nz->total_sumsq, f32(NF_TOTAL_SUMSQ), n);
        small_copy<RESTORE>(nz->total_count, f32(NF_TOTAL_COUNT), 1);
        small_copy<RESTORE>(nz->mean, f32(NF_MEAN), n);
        small_copy<RESTORE>(nz->std, reinterpret_cast<double *>(A.base + A.off[s0 + NF_STD]), n);
    }
    small_copy<RESTORE>(A.rng->key, reinterpret_cast<uint32_t *>(A.base + A.off[ST_RNG_KEY]), MT_N);
    small_copy<RESTORE>(&A.rng->pos, reinterpret_cast<int32_t *>(A.base + A.off[ST_RNG_POS]), 1);
    small_copy<RESTORE>(&A.st->step, reinterpret_cast<long long *>(A.base + A.off[ST_ADAM_STEP]), 1);
    long long *cnt = reinterpret_cast<long long *>(A.base + A.off[ST_BUF_COUNTERS]);
    if (threadIdx.x == 0) {
        if (RESTORE) {
            A.meta->current_size = cnt[0];
            A.meta->n_transitions_stored = cnt[1];
            A.st->n_logged = 0;   // the loss log is not part of a state: hp_agent_get_losses reports updates made since
        } else {
            cnt[0] = A.meta->current_size;
            cnt[1] = A.meta->n_transitions_stored;
        }
    }
}

// ---- delta: which slots were written since a capture, and their rows
// Dirty scan: the slots in [0, cs) whose stamp is > since, ascending.  Count per chunk of DS_CHUNK slots, exclusive scan of the
// counts by one workgroup (capacities go to 2^31 slots = 2^20 chunks; 5 000 slots are 3), emit.  Within a chunk a thread looks at
// slot chunk * DS_CHUNK + it * 256 + tid, so (it, wave, lane) order is slot order.
struct DirtyArgs {
    const uint32_t *stamp;
    long long cs;          // slots scanned (the buffer's current_size)
    uint32_t since;
    long long max_dirty;   // room in `slots`
    long long *counts;     // [n_chunks]: counts, then (k_dirty_scan) the number of dirty slots in front of each chunk
    long long n_chunks;
    long long *hdr;        // [0] n_dirty, [1] overflow
    long long *slots;
};

__device__ __forceinline__ bool dirty_at(const DirtyArgs &A, long long slot) { return slot < A.cs && A.stamp[slot] > A.since; }

__global__ __launch_bounds__(DS_CHUNK_THREADS) void k_dirty_count(const DirtyArgs A) {
    __shared__ int wave_n[DS_CHUNK_THREADS / 64];
    const long long first = (long long)blockIdx.x * DS_CHUNK;
    int n = 0;
#pragma unroll
    for (int it = 0; it < DS_CHUNK_ITEMS; ++it)
        n += __popcll(__ballot(dirty_at(A, first + it * DS_CHUNK_THREADS + threadIdx.x)));
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) A.counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

__global__ __launch_bounds__(256) void k_dirty_scan(const DirtyArgs A) {
    __shared__ long long wave_tot[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    long long carry = 0;
    for (long long base = 0; base < A.n_chunks; base += 256) {
        const long long j = base + tid;
        const long long v = j < A.n_chunks ? A.counts[j] : 0;
        long long x = v;
        for (int o = 1; o < 64; o <<= 1) {
            const long long y = __shfl_up(x, o);
            if (lane >= o) x += y;
        }
        if (lane == 63) wave_tot[wave] = x;
        __syncthreads();
        long long pre = 0;
        for (int k = 0; k < wave; ++k) pre += wave_tot[k];
        if (j < A.n_chunks) A.counts[j] = carry + pre + x - v;
        carry += wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
        __syncthreads();
    }
    if (tid == 0) {
        A.hdr[0] = carry;
        A.hdr[1] = carry > A.max_dirty ? 1 : 0;   // the caller's bound was wrong: nothing past it is emitted, fetch refuses
    }
}

__global__ __launch_bounds__(DS_CHUNK_THREADS) void k_dirty_emit(const DirtyArgs A) {
    __shared__ int wave_n[DS_CHUNK_ITEMS][DS_CHUNK_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long first = (long long)blockIdx.x * DS_CHUNK;
    u64 bal[DS_CHUNK_ITEMS];
#pragma unroll
    for (int it = 0; it < DS_CHUNK_ITEMS; ++it) {
        bal[it] = __ballot(dirty_at(A, first + it * DS_CHUNK_THREADS + tid));
        if (lane == 0) wave_n[it][wave] = __popcll(bal[it]);
    }
    __syncthreads();
    long long pos = A.counts[blockIdx.x];
#pragma unroll
    for (int it = 0; it < DS_CHUNK_ITEMS; ++it) {
        int before = 0, all = 0;
        for (int w = 0; w < DS_CHUNK_THREADS / 64; ++w) {
            if (w < wave) before += wave_n[it][w];
            all += wave_n[it][w];
        }
        if ((bal[it] >> lane) & 1ull) {
            const long long at = pos + before + __popcll(bal[it] & ((1ull << lane) - 1ull));
            if (at < A.max_dirty) A.slots[at] = first + it * DS_CHUNK_THREADS + tid;
        }
        pos += all;
    }
}

// Row pack: episode e of the delta = the rows of slot slots[e], for the four arrays.  DS_PACK_PARTS workgroups share an episode;
// the grid strides over the n_dirty episodes the scan found (read from the header: the host does not know the count).  Rows start
// on 8-byte boundaries, (T + 1) * dim doubles long: where source and destination agree on their offset mod 16 the body is 16-byte
// loads and stores (behind a leading word when both sit at 8 mod 16), otherwise word by word.
#define DS_PACK_PARTS 4
struct PackArgs {
    const long long *hdr, *slots;
    long long max_dirty;
    const double *src[4];
    double *dst[4];
    long long ep[4];
};

__device__ __forceinline__ void copy_row(double *__restrict__ d, const double *__restrict__ s, long long n, long long t0, long long step) {
    const unsigned ms = (unsigned)(((uintptr_t)s >> 3) & 1u), md = (unsigned)(((uintptr_t)d >> 3) & 1u);
    if (ms != md) {
        for (long long k = t0; k < n; k += step) d[k] = s[k];
        return;
    }
    const long long head = (ms && n > 0) ? 1 : 0, npairs = (n - head) / 2;
    const f64x2 *sv = reinterpret_cast<const f64x2 *>(s + head);
    f64x2 *dv = reinterpret_cast<f64x2 *>(d + head);
    for (long long p = t0; p < npairs; p += step) dv[p] = sv[p];
    if (t0 == 0) {
        if (head) d[0] = s[0];
        if ((n - head) & 1) d[n - 1] = s[n - 1];
    }
}

__global__ __launch_bounds__(256) void k_delta_pack(const PackArgs A) {
    const long long n = A.hdr[0] < A.max_dirty ? A.hdr[0] : A.max_dirty;
    const int part = blockIdx.x % DS_PACK_PARTS;
    const long long t0 = (long long)part * blockDim.x + threadIdx.x, step = (long long)DS_PACK_PARTS * blockDim.x;
    for (long long e = blockIdx.x / DS_PACK_PARTS; e < n; e += gridDim.x / DS_PACK_PARTS) {
        const long long slot = A.slots[e];
#pragma unroll
        for (int k = 0; k < 4; ++k) copy_row(A.dst[k] + e * A.ep[k], A.src[k] + slot * A.ep[k], A.ep[k], t0, step);
    }
}

// a capture records the buffer's epoch and advances it, in stream order: what is scattered behind it is stamped with the new value
__global__ void k_epoch_advance(uint32_t *epoch, long long *hdr, long long since) {
    const uint32_t e = *epoch;
    if (hdr) {
        hdr[2] = (long long)e;
        hdr[3] = since;
    }
    *epoch = e + 1u;
}

// ------------------------------------------------------------------------------- host side
static FlatMap flat_map(const hp_agent *a, bool critic) {
    const NetLayout &l = critic ? a->lc : a->la;
    FlatMap m;
    m.w1 = l.w1; m.b1 = l.b1; m.w2 = l.w2; m.b2 = l.b2; m.w3 = l.w3; m.b3 = l.b3; m.w4 = l.w4; m.b4 = l.b4;
    m.K1 = l.K1; m.H = a->H; m.xdim = a->xdim; m.act_off = a->act_off;
    m.in1 = critic ? a->xdim + a->cfg.act_dim : a->xdim;
    m.out4 = critic ? 1 : a->cfg.act_dim;
    m.base = critic ? a->la.total : 0;
    m.n = m.H * m.in1 + m.H + 2 * (m.H * m.H + m.H) + m.out4 * m.H + m.out4;
    return m;
}

static const char *const k_norm_field[NORM_FIELDS] = {"local_sum", "local_sumsq", "local_count", "total_sum",
                                                      "total_sumsq", "total_count", "mean", "std"};
static const int k_elem_bytes[5] = {4, 8, 8, 4, 4};

static int n_sections(bool delta) { return delta ? DS_SECTIONS : ST_SECTIONS; }

// the buffer's four row arrays: where they live and how many doubles an episode has in each
struct BufRows {
    double *dev[4];
    long long ep[4];
};
static BufRows buffer_rows(const hp_buffer *b) {
    return {{b->d_obs, b->d_ag, b->d_g, b->d_act},
            {(long long)b->ep_obs(), (long long)b->ep_ag(), (long long)b->ep_g(), (long long)b->ep_act()}};
}

// THE layout of a training state (state.h has the section order): the small sections, then the buffer -- of a full state as the
// rows of its first n_episodes episodes, of a delta as header, slot list and packed rows with room for n_episodes dirty ones --
// then the counters.  Fills S[0 .. n_sections(delta)) and returns the blob's size.
static size_t state_layout(const hp_agent *a, const hp_buffer *b, const hp_norm *on, const hp_norm *gn, bool delta,
                           int64_t n_episodes, hp_state_section *S) {
    const int nsec = n_sections(delta);
    memset(S, 0, sizeof(hp_state_section) * nsec);
    auto set = [&](int i, const char *name, int dtype, int64_t count) {
        snprintf(S[i].name, sizeof(S[i].name), "%s", name);
        S[i].dtype = dtype;
        S[i].elem_bytes = k_elem_bytes[dtype];
        S[i].count = count;
    };
    const int64_t na = flat_map(a, false).n, nc = flat_map(a, true).n;
    static const char *const k_flat[8] = {"actor", "critic", "actor_target", "critic_target",
                                          "adam_actor_m", "adam_actor_v", "adam_critic_m", "adam_critic_v"};
    for (int v = 0; v < 8; ++v) set(ST_ACTOR + v, k_flat[v], SD_F32, (v == 1 || v == 3 || v >= 6) ? nc : na);   // as k_state_flat
    set(ST_ADAM_STEP, "adam_step", SD_I64, 1);
    for (int k = 0; k < 2; ++k)
        for (int f = 0; f < NORM_FIELDS; ++f) {
            char name[32];
            snprintf(name, sizeof(name), "%s_%s", k ? "g_norm" : "o_norm", k_norm_field[f]);
            const bool one = f == NF_LOCAL_COUNT || f == NF_TOTAL_COUNT;
            set((k ? ST_GNORM : ST_ONORM) + f, name, f == NF_STD ? SD_F64 : SD_F32, one ? 1 : (k ? gn->size : on->size));
        }
    set(ST_RNG_KEY, "rng_key", SD_U32, MT_N);
    set(ST_RNG_POS, "rng_pos", SD_I32, 1);
    static const char *const k_rows[2][4] = {{"buffer_obs", "buffer_ag", "buffer_g", "buffer_actions"},
                                             {"buffer_delta_obs", "buffer_delta_ag", "buffer_delta_g", "buffer_delta_actions"}};
    if (delta) {
        set(DS_HEADER, "buffer_delta_header", SD_I64, 4);
        set(DS_SLOTS, "buffer_delta_slots", SD_I64, n_episodes);
    }
    const BufRows R = buffer_rows(b);
    for (int k = 0; k < 4; ++k) set((delta ? DS_OBS : ST_BUF_OBS) + k, k_rows[delta][k], SD_F64, n_episodes * R.ep[k]);
    set(nsec - 1, "buffer_counters", SD_I64, 2);
    size_t off = 0;
    for (int i = 0; i < nsec; ++i) {
        S[i].offset = (int64_t)off;
        off += ((size_t)S[i].count * S[i].elem_bytes + ST_ALIGN - 1) / ST_ALIGN * ST_ALIGN;
    }
    return off;
}

static int state_handles(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, hp_rng *rng, const char *who) {
    HP_REQUIRE(a && b && on && gn && rng, HP_ERR_INVALID, "%s: null handle", who);
    HP_REQUIRE(b->ctx == a->ctx && on->ctx == a->ctx && gn->ctx == a->ctx && rng->ctx == a->ctx, HP_ERR_INVALID,
               "%s: the handles belong to different contexts", who);
    HP_REQUIRE(b->obs_dim == a->cfg.obs_dim && b->goal_dim == a->cfg.goal_dim && b->act_dim == a->cfg.act_dim, HP_ERR_INVALID,
               "%s: buffer dimensions do not match the agent", who);
    HP_REQUIRE(on->size == a->cfg.obs_dim && gn->size == a->cfg.goal_dim, HP_ERR_INVALID,
               "%s: normalizer sizes do not match the agent", who);
    return HP_OK;
}

static int arena_get(hp_agent *a, StateArena **out) {
    if (!a->state) {
        StateArena *A = new StateArena();
        a->state = A;
        HP_CHECK_HIP(hipStreamCreateWithFlags(&A->drain, hipStreamNonBlocking));
        HP_CHECK_HIP(hipEventCreateWithFlags(&A->captured, hipEventDisableTiming));
        HP_CHECK_HIP(hipEventCreateWithFlags(&A->drained, hipEventDisableTiming));
        HP_CHECK_HIP(hipMalloc((void **)&A->d_sums, sizeof(u64) * 2 * DS_SECTIONS));
        HP_CHECK_HIP(hipHostMalloc((void **)&A->pin_sums, sizeof(u64) * 2 * DS_SECTIONS, hipHostMallocDefault));
    }
    *out = a->state;
    return HP_OK;
}

// grow the snapshot arena and, for a capture, its pinned copy (nobody reads them: the caller has made sure no drain is in flight)
static int arena_ensure(StateArena *A, size_t need, bool pinned) {
    if (need > A->dev_bytes) {
        if (A->dev) (void)hipFree(A->dev);
        A->dev = nullptr;
        A->dev_bytes = 0;
        HP_CHECK_HIP(hipMalloc((void **)&A->dev, need));
        A->dev_bytes = need;
    }
    if (pinned && need > A->pin_bytes) {
        if (A->pin) (void)hipHostFree(A->pin);
        A->pin = nullptr;
        A->pin_bytes = 0;
        HP_CHECK_HIP(hipHostMalloc((void **)&A->pin, need, hipHostMallocDefault));
        A->pin_bytes = need;
    }
    return HP_OK;
}

// workgroups of a checksum over nwords 8-byte words: four 16-byte loads per lane and trip
static unsigned checksum_grid(u64 nwords) {
    return (unsigned)std::min<u64>(std::max<u64>((nwords / 2 + 256 * 4 - 1) / (256 * 4), 1), 2048);
}

static int launch_checksum(const void *dev, size_t bytes, u64 *d_out, hipStream_t s, int blocks = 0) {
    const u64 nwords = bytes / 8;
    HP_KLOG("k_checksum");
    hipLaunchKernelGGL(k_checksum, dim3(blocks > 0 ? (unsigned)blocks : checksum_grid(nwords)), dim3(256), 0, s,
                       static_cast<const u64 *>(dev), nwords, (unsigned)(bytes % 8), d_out);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// The sums of the nsec sections of the layout S in the arena, on stream s: whole sections, but of a delta (hdr = its header in the
// arena) the used prefix of the slot list and of the four row sections -- nothing at all where there is no room for a slot.
static int checksum_layout(StateArena *A, const hp_state_section *S, int nsec, hipStream_t s, const long long *hdr,
                           int64_t max_dirty) {
    HP_CHECK_HIP(hipMemsetAsync(A->d_sums, 0, sizeof(u64) * 2 * nsec, s));
    for (int i = 0; i < nsec; ++i) {
        if (!hdr || i < DS_SLOTS || i > DS_ACT) {
            HP_TRY(launch_checksum(A->dev + S[i].offset, (size_t)S[i].count * S[i].elem_bytes, A->d_sums + 2 * i, s));
            continue;
        }
        if (max_dirty == 0) continue;
        HP_KLOG("k_checksum_prefix");
        hipLaunchKernelGGL(k_checksum_prefix, dim3(checksum_grid((u64)S[i].count)), dim3(256), 0, s,
                           reinterpret_cast<const u64 *>(A->dev + S[i].offset), hdr, (u64)(S[i].count / max_dirty),   // words per episode
                           (long long)max_dirty, A->d_sums + 2 * i);
        HP_CHECK_HIP(hipGetLastError());
    }
    return HP_OK;
}

// k_state_flat + k_state_small between the live objects and the layout S at `base`, on the learner's stream; `counters` is the
// index of S's buffer_counters section (the small sections sit at the same indices in both kinds of state).  A restore rebuilds
// every derived copy of the parameters between the two, as hp_agent_set_params / hp_agent_sync_targets do.
template <bool RESTORE>
static int launch_state_pair(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, hp_rng *rng, char *base, const hp_state_section *S,
                             int counters) {
    hipStream_t s = a->ctx->stream;
    FlatArgs F;
    float *arena[8] = {a->params, a->params, a->targets, a->targets, a->adam_m, a->adam_v, a->adam_m, a->adam_v};
    for (int v = 0; v < 8; ++v) {
        F.arena[v] = arena[v];
        F.flat[v] = reinterpret_cast<float *>(base + S[ST_ACTOR + v].offset);
    }
    F.m[0] = flat_map(a, false);
    F.m[1] = flat_map(a, true);
    const int nmax = std::max(F.m[0].n, F.m[1].n);
    if (!RESTORE) HP_KLOG("k_state_flat");
    hipLaunchKernelGGL(k_state_flat<RESTORE>, dim3((unsigned)((nmax + 255) / 256), 8), dim3(256), 0, s, F);
    HP_CHECK_HIP(hipGetLastError());
    if (RESTORE) {
        HP_TRY(enqueue_relayout(a, false));
        HP_TRY(enqueue_relayout(a, true));
    }
    SmallArgs M;
    M.nz[0] = on->d; M.nz[1] = gn->d;
    M.size[0] = on->size; M.size[1] = gn->size;
    M.rng = rng->d_state; M.st = a->d_state; M.meta = b->d_meta; M.base = base;
    for (int i = 0; i < ST_SECTIONS; ++i) M.off[i] = S[i].offset;
    M.off[ST_BUF_COUNTERS] = S[counters].offset;
    if (!RESTORE) HP_KLOG("k_state_small");
    hipLaunchKernelGGL(k_state_small<RESTORE>, dim3(1), dim3(256), 0, s, M);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// The dirty scan of `cs` slots of b on stream s: hdr[0] = n_dirty, hdr[1] = overflow, slots[0 .. min(n_dirty, max_dirty)).
static int launch_dirty_scan(hp_buffer *b, int64_t cs, uint32_t since, int64_t max_dirty, long long *hdr, long long *slots,
                             hipStream_t s) {
    DirtyArgs D;
    D.stamp = b->d_slot_epoch;
    D.cs = cs;
    D.since = since;
    D.max_dirty = max_dirty;
    D.n_chunks = (cs + DS_CHUNK - 1) / DS_CHUNK;
    HP_TRY(b->dirty_counts.ensure(std::max<size_t>((size_t)D.n_chunks, 1) * sizeof(long long)));
    D.counts = b->dirty_counts.as<long long>();
    D.hdr = hdr;
    D.slots = slots;
    if (D.n_chunks > 0) {
        HP_KLOG("k_dirty_count");
        hipLaunchKernelGGL(k_dirty_count, dim3((unsigned)D.n_chunks), dim3(DS_CHUNK_THREADS), 0, s, D);
        HP_CHECK_HIP(hipGetLastError());
    }
    HP_KLOG("k_dirty_scan");
    hipLaunchKernelGGL(k_dirty_scan, dim3(1), dim3(256), 0, s, D);
    HP_CHECK_HIP(hipGetLastError());
    if (D.n_chunks > 0 && max_dirty > 0) {
        HP_KLOG("k_dirty_emit");
        hipLaunchKernelGGL(k_dirty_emit, dim3((unsigned)D.n_chunks), dim3(DS_CHUNK_THREADS), 0, s, D);
        HP_CHECK_HIP(hipGetLastError());
    }
    return HP_OK;
}

void state_arena_destroy(hp_agent *a) {
    StateArena *A = a->state;
    if (!A) return;
    if (A->drain) (void)hipStreamSynchronize(A->drain);
    if (A->dev) (void)hipFree(A->dev);
    if (A->d_sums) (void)hipFree(A->d_sums);
    if (A->pin) (void)hipHostFree(A->pin);
    if (A->pin_sums) (void)hipHostFree(A->pin_sums);
    if (A->captured) (void)hipEventDestroy(A->captured);
    if (A->drained) (void)hipEventDestroy(A->drained);
    if (A->drain) (void)hipStreamDestroy(A->drain);
    delete A;
    a->state = nullptr;
}

// --------------------------------------------------------------------------------- C ABI
// hp_state_layout (n_episodes = current_size, < 0: the buffer's) and hp_state_layout_delta (n_episodes = max_dirty)
static int layout_entry(const char *who, bool delta, hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, int64_t n_episodes,
                        hp_state_section *out, int32_t *n, size_t *total_bytes) {
    HP_REQUIRE(a && b && on && gn && n, HP_ERR_INVALID, "%s: null argument", who);
    HP_SERIALISE(a);
    if (delta) {
        HP_REQUIRE(n_episodes >= 0 && n_episodes <= b->size, HP_ERR_INVALID, "%s: max_dirty %lld outside [0, %lld]", who,
                   (long long)n_episodes, (long long)b->size);
    } else {
        if (n_episodes < 0) n_episodes = b->current_size;
        HP_REQUIRE(n_episodes <= b->size, HP_ERR_INVALID, "%s: current_size %lld exceeds the buffer's capacity %lld", who,
                   (long long)n_episodes, (long long)b->size);
    }
    hp_state_section S[DS_SECTIONS];
    const int nsec = n_sections(delta);
    const size_t total = state_layout(a, b, on, gn, delta, n_episodes, S);
    if (out) {
        HP_REQUIRE(*n >= nsec, HP_ERR_INVALID, "%s: room for %d sections, %d needed", who, *n, nsec);
        memcpy(out, S, sizeof(hp_state_section) * nsec);
    }
    *n = nsec;
    if (total_bytes) *total_bytes = total;
    return HP_OK;
}

// Both kinds of capture.  delta: the buffer as the slots stamped since the capture `since` (room for max_dirty episodes).
static int state_capture(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, hp_rng *rng, bool delta, uint32_t since,
                         int64_t max_dirty, uint64_t *ticket, size_t *bytes) {
    const char *who = delta ? "hp_state_capture_delta" : "hp_state_capture";
    HP_TRY(state_handles(a, b, on, gn, rng, who));
    HP_REQUIRE(ticket, HP_ERR_INVALID, "%s: null ticket", who);
    HP_SERIALISE(a);
    HP_TRY(agent_check_fault(a, who));
    StateArena *A = nullptr;
    HP_TRY(arena_get(a, &A));
    HP_REQUIRE(!A->pending, HP_ERR_STATE, "%s: the capture with ticket %llu has not been fetched yet "
               "(hp_state_fetch; a null host_out abandons it)", who, (unsigned long long)A->ticket);
    HP_REQUIRE(b->epoch < 0xFFFFFFFFu, HP_ERR_STATE, "%s: the buffer's capture epoch has reached 2^32 - 1", who);
    hipStream_t s = a->ctx->stream;
    const int64_t cs = b->current_size;
    if (delta) {
        HP_REQUIRE(since >= b->min_since, HP_ERR_STATE, "hp_state_capture_delta: since_epoch %u is older than the last restore "
                   "(min_since %u): the rows that changed before it are not known any more", since, b->min_since);
        HP_REQUIRE(since < b->epoch, HP_ERR_STATE, "hp_state_capture_delta: since_epoch %u is not a capture of this buffer "
                   "(its epoch is %u)", since, b->epoch);
        HP_REQUIRE(max_dirty >= 0 && max_dirty <= cs, HP_ERR_INVALID, "hp_state_capture_delta: max_dirty %lld outside [0, %lld]",
                   (long long)max_dirty, (long long)cs);
    }
    hp_state_section S[DS_SECTIONS];
    const int nsec = n_sections(delta);
    const size_t total = state_layout(a, b, on, gn, delta, delta ? max_dirty : cs, S);
    // the previous ticket was fetched, so its drain is over: arena and pinned copy are free
    HP_TRY(arena_ensure(A, total, true));
    // learner's stream: the snapshot itself, nothing else
    HP_TRY(launch_state_pair<false>(a, b, on, gn, rng, A->dev, S, nsec - 1));
    const BufRows R = buffer_rows(b);
    long long *hdr = nullptr;
    if (delta) {
        hdr = reinterpret_cast<long long *>(A->dev + S[DS_HEADER].offset);
        long long *slots = reinterpret_cast<long long *>(A->dev + S[DS_SLOTS].offset);
        HP_TRY(launch_dirty_scan(b, cs, since, max_dirty, hdr, slots, s));
        if (max_dirty > 0) {
            PackArgs P;
            P.hdr = hdr; P.slots = slots; P.max_dirty = max_dirty;
            for (int k = 0; k < 4; ++k) {
                P.src[k] = R.dev[k];
                P.dst[k] = reinterpret_cast<double *>(A->dev + S[DS_OBS + k].offset);
                P.ep[k] = R.ep[k];
            }
            HP_KLOG("k_delta_pack");
            hipLaunchKernelGGL(k_delta_pack, dim3((unsigned)(std::min<int64_t>(max_dirty, 4096) * DS_PACK_PARTS)), dim3(256), 0, s, P);
            HP_CHECK_HIP(hipGetLastError());
        }
    } else {
        for (int k = 0; k < 4 && cs > 0; ++k)
            HP_CHECK_HIP(hipMemcpyAsync(A->dev + S[ST_BUF_OBS + k].offset, R.dev[k], (size_t)S[ST_BUF_OBS + k].count * 8,
                                        hipMemcpyDeviceToDevice, s));
    }
    HP_KLOG("k_epoch_advance");
    hipLaunchKernelGGL(k_epoch_advance, dim3(1), dim3(1), 0, s, b->d_epoch, hdr, (long long)since);
    HP_CHECK_HIP(hipGetLastError());
    A->capture_epoch = b->epoch++;
    HP_CHECK_HIP(hipEventRecord(A->captured, s));
    // drain stream: checksums of the snapshot, then the snapshot and the sums to pinned memory
    HP_CHECK_HIP(hipStreamWaitEvent(A->drain, A->captured, 0));
    HP_TRY(checksum_layout(A, S, nsec, A->drain, hdr, max_dirty));
    for (size_t off = 0; off < total; off += ST_DRAIN_CHUNK)
        HP_CHECK_HIP(hipMemcpyAsync(A->pin + off, A->dev + off, std::min<size_t>(ST_DRAIN_CHUNK, total - off),
                                    hipMemcpyDeviceToHost, A->drain));
    HP_CHECK_HIP(hipMemcpyAsync(A->pin_sums, A->d_sums, sizeof(u64) * 2 * nsec, hipMemcpyDeviceToHost, A->drain));
    HP_CHECK_HIP(hipEventRecord(A->drained, A->drain));
    A->pending = true;
    A->bytes = total;
    A->delta = delta;
    A->hdr_off = delta ? (size_t)S[DS_HEADER].offset : 0;
    *ticket = ++A->ticket;
    if (bytes) *bytes = total;
    return HP_OK;
}

extern "C" {

int hp_state_layout(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, int64_t current_size, hp_state_section *out,
                    int32_t *n, size_t *total_bytes) {
    return layout_entry("hp_state_layout", false, a, b, on, gn, current_size, out, n, total_bytes);
}

int hp_state_layout_delta(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, int64_t max_dirty, hp_state_section *out, int32_t *n,
                          size_t *total_bytes) {
    return layout_entry("hp_state_layout_delta", true, a, b, on, gn, max_dirty, out, n, total_bytes);
}

int hp_state_capture(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, hp_rng *rng, uint64_t *ticket, size_t *bytes) {
    return state_capture(a, b, on, gn, rng, false, 0, 0, ticket, bytes);
}

int hp_state_capture_delta(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, hp_rng *rng, uint32_t since_epoch, int64_t max_dirty,
                           uint64_t *ticket, size_t *bytes) {
    return state_capture(a, b, on, gn, rng, true, since_epoch, max_dirty, ticket, bytes);
}

int hp_state_epochs(hp_agent *a, hp_buffer *b, uint32_t *capture_epoch, uint32_t *epoch, uint32_t *min_since) {
    HP_REQUIRE(a && b && b->ctx == a->ctx, HP_ERR_INVALID, "hp_state_epochs: null handle, or handles of different contexts");
    HP_SERIALISE(a);
    if (capture_epoch) *capture_epoch = a->state ? a->state->capture_epoch : 0u;
    if (epoch) *epoch = b->epoch;
    if (min_since) *min_since = b->min_since;
    return HP_OK;
}

int hp_state_fetch(hp_agent *a, uint64_t ticket, int32_t wait, void *host_out, size_t bytes, uint64_t *sums, int32_t *done) {
    HP_REQUIRE(a, HP_ERR_INVALID, "hp_state_fetch: null handle");
    StateArena *A = nullptr;
    {
        HP_SERIALISE(a);
        A = a->state;
        HP_REQUIRE(A && A->pending && ticket == A->ticket, HP_ERR_STATE, "hp_state_fetch: ticket %llu is not the pending capture",
                   (unsigned long long)ticket);
        HP_REQUIRE(!host_out || bytes == A->bytes, HP_ERR_INVALID, "hp_state_fetch: the capture holds %zu bytes, the caller gave %zu",
                   A->bytes, bytes);
    }
    // outside the context lock: the trainer keeps enqueueing meanwhile
    if (wait || !host_out) HP_CHECK_HIP(hipEventSynchronize(A->drained));
    else {
        const hipError_t q = hipEventQuery(A->drained);
        if (q == hipErrorNotReady) {
            (void)hipGetLastError();
            if (done) *done = 0;
            return HP_OK;
        }
        HP_CHECK_HIP(q);
    }
    // (the pinned copy cannot change under this: a new capture is refused while this ticket is pending)
    long long hdr[2] = {0, 0};
    if (A->delta) memcpy(hdr, A->pin + A->hdr_off, sizeof(hdr));
    if (host_out && !hdr[1]) {
        memcpy(host_out, A->pin, A->bytes);
        if (sums) memcpy(sums, A->pin_sums, sizeof(u64) * 2 * n_sections(A->delta));
    }
    {
        HP_SERIALISE(a);
        A->pending = false;
    }
    HP_REQUIRE(!host_out || !hdr[1], HP_ERR_STATE, "hp_state_fetch: the delta found %lld dirty slots, more than the max_dirty it was "
               "sized for: nothing is delivered, the ticket is retired", hdr[0]);
    if (done) *done = 1;
    return HP_OK;
}

int hp_state_restore(hp_agent *a, hp_buffer *b, hp_norm *on, hp_norm *gn, hp_rng *rng, const hp_state_dims *dims,
                     const void *host_in, size_t bytes, const uint64_t *sums) {
    HP_TRY(state_handles(a, b, on, gn, rng, "hp_state_restore"));
    HP_REQUIRE(dims && host_in && sums, HP_ERR_INVALID, "hp_state_restore: null argument");
    HP_SERIALISE(a);
    HP_TRY(agent_check_fault(a, "hp_state_restore"));
#define ST_FIELD(name, got, want)                                                                                   \
    HP_REQUIRE((long long)(got) == (long long)(want), HP_ERR_INVALID, "hp_state_restore: %s of the state is %lld, the receiver has %lld", \
               name, (long long)(got), (long long)(want))
    ST_FIELD("obs", dims->obs_dim, a->cfg.obs_dim);
    ST_FIELD("goal", dims->goal_dim, a->cfg.goal_dim);
    ST_FIELD("action", dims->act_dim, a->cfg.act_dim);
    ST_FIELD("hidden", dims->hidden, a->H);
    ST_FIELD("T", dims->T, b->T);
    ST_FIELD("capacity", dims->capacity, b->size);   // the overflow slot draws depend on it (replay_buffer.py:57-71)
#undef ST_FIELD
    const int64_t cs = dims->current_size;
    HP_REQUIRE(cs >= 0 && cs <= b->size, HP_ERR_INVALID, "hp_state_restore: current_size %lld outside [0, %lld]", (long long)cs,
               (long long)b->size);
    hp_state_section S[ST_SECTIONS];
    const size_t total = state_layout(a, b, on, gn, false, cs, S);
    HP_REQUIRE(bytes == total, HP_ERR_INVALID, "hp_state_restore: a state of %lld episodes is %zu bytes, the caller gave %zu",
               (long long)cs, total, bytes);
    const char *in = static_cast<const char *>(host_in);
    long long cnt[2];
    int32_t pos;
    memcpy(cnt, in + S[ST_BUF_COUNTERS].offset, sizeof(cnt));
    memcpy(&pos, in + S[ST_RNG_POS].offset, sizeof(pos));
    HP_REQUIRE(cnt[0] == cs, HP_ERR_INVALID, "hp_state_restore: buffer_counters says current_size %lld, the header %lld", cnt[0],
               (long long)cs);
    HP_REQUIRE(pos >= 0 && pos <= MT_N, HP_ERR_INVALID, "hp_state_restore: rng_pos %d outside [0, 624]", pos);
    HP_REQUIRE(b->epoch < 0xFFFFFFFDu, HP_ERR_STATE, "hp_state_restore: the buffer's capture epoch has reached 2^32 - 1");
    StateArena *A = nullptr;
    HP_TRY(arena_get(a, &A));
    // a capture still draining reads the arena: let it finish (its pinned copy stays fetchable)
    if (A->pending) HP_CHECK_HIP(hipEventSynchronize(A->drained));
    hipStream_t s = a->ctx->stream;
    HP_TRY(arena_ensure(A, total, false));
    // 1. upload into the arena and sum it THERE: nothing live is touched before the sums agree with the caller's
    HP_CHECK_HIP(hipMemcpyAsync(A->dev, host_in, total, hipMemcpyHostToDevice, s));
    HP_TRY(checksum_layout(A, S, ST_SECTIONS, s, nullptr, 0));
    u64 got[2 * ST_SECTIONS];
    HP_CHECK_HIP(hipMemcpyAsync(got, A->d_sums, sizeof(got), hipMemcpyDeviceToHost, s));
    HP_CHECK_HIP(hipStreamSynchronize(s));
    for (int i = 0; i < ST_SECTIONS; ++i)
        HP_REQUIRE(got[2 * i] == sums[2 * i] && got[2 * i + 1] == sums[2 * i + 1], HP_ERR_INVALID,
                   "hp_state_restore: checksum of '%s' on the device is (%016llx, %016llx), the state says (%016llx, %016llx): nothing "
                   "was restored", S[i].name, got[2 * i], got[2 * i + 1], (u64)sums[2 * i], (u64)sums[2 * i + 1]);
    // 2. commit.  Parameters, targets and optimizer state into the arenas, then every derived copy as hp_agent_set_params /
    // hp_agent_sync_targets rebuild them
    HP_TRY(launch_state_pair<true>(a, b, on, gn, rng, A->dev, S, ST_BUF_COUNTERS));
    const BufRows R = buffer_rows(b);
    for (int k = 0; k < 4 && cs > 0; ++k)
        HP_CHECK_HIP(hipMemcpyAsync(R.dev[k], A->dev + S[ST_BUF_OBS + k].offset, (size_t)S[ST_BUF_OBS + k].count * 8,
                                    hipMemcpyDeviceToDevice, s));
    HP_TRY(buffer_launch_pack_range(b, 0, cs));   // throughput rows, when the receiver has them
    b->current_size = cs;
    b->n_transitions_stored = cnt[1];
    b->staged_n = 0;                 // staged episodes are not part of a state
    // Delta states: which slots changed before now is not known any more.  The stamps start over; the restored state stands for a
    // capture with an epoch larger than any handed out before (min_since), and what is stored from here on is stamped above it.
    HP_CHECK_HIP(hipMemsetAsync(b->d_slot_epoch, 0, (size_t)b->size * sizeof(uint32_t), s));
    b->min_since = b->epoch + 1u;
    b->epoch = b->min_since + 1u;
    HP_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)b->d_epoch, (int)b->epoch, 1, s));
    // a policy snapshot taken before now is a copy of parameters that no longer exist: hp_agent_act_snapshot must not serve it
    a->snap_cur = -1;
    a->snap_pending = -1;
    // The cached update and cycle graphs stay valid: they bake in addresses (unchanged) and read every counter from device
    // memory (BufMeta, AgentDevState, MtState) at run time.
    HP_CHECK_HIP(hipStreamSynchronize(s));
    return HP_OK;
}

int hp_state_debug_dirty_scan(hp_buffer *b, const uint32_t *stamps_host, int64_t current_size, uint32_t since, int64_t max_dirty,
                              int64_t *slots_out, int64_t *n_dirty, int32_t *overflow) {
    HP_REQUIRE(b && stamps_host && n_dirty && (slots_out || max_dirty == 0), HP_ERR_INVALID, "hp_state_debug_dirty_scan: null argument");
    HP_REQUIRE(current_size >= 0 && current_size <= b->size && max_dirty >= 0 && max_dirty <= b->size, HP_ERR_INVALID,
               "hp_state_debug_dirty_scan: current_size / max_dirty outside [0, %lld]", (long long)b->size);
    HP_SERIALISE(b);
    hipStream_t s = b->ctx->stream;
    DevBuf out;   // header (2 words, padded to 4) | slots
    HP_TRY(out.ensure((4 + std::max<size_t>((size_t)max_dirty, 1)) * sizeof(long long)));
    long long *hdr = out.as<long long>(), *slots = hdr + 4;
    long long h[2] = {0, 0};
    int st = HP_OK;
    hipError_t e = hipMemcpyAsync(b->d_slot_epoch, stamps_host, (size_t)b->size * sizeof(uint32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) st = launch_dirty_scan(b, current_size, since, max_dirty, hdr, slots, s);
    if (e == hipSuccess && st == HP_OK) e = hipMemcpyAsync(h, hdr, sizeof(h), hipMemcpyDeviceToHost, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    const long long used = h[0] < max_dirty ? h[0] : max_dirty;
    if (e == hipSuccess && st == HP_OK && used > 0) e = hipMemcpy(slots_out, slots, (size_t)used * sizeof(long long), hipMemcpyDeviceToHost);
    out.release();
    HP_TRY(st);
    HP_CHECK_HIP(e);
    *n_dirty = h[0];
    if (overflow) *overflow = (int32_t)h[1];
    return HP_OK;
}

int hp_state_checksum_dev(hp_ctx *ctx, const void *dev, size_t bytes, int32_t blocks, uint64_t *out2) {
    HP_REQUIRE(ctx && out2 && (dev || bytes == 0), HP_ERR_INVALID, "hp_state_checksum_dev: null argument");
    HP_REQUIRE(((uintptr_t)dev & 7u) == 0, HP_ERR_INVALID, "hp_state_checksum_dev: the data must start on an 8-byte boundary");
    HP_REQUIRE(blocks >= 0 && blocks <= 65536, HP_ERR_INVALID, "hp_state_checksum_dev: blocks must be in [0, 65536]");
    CtxGuard guard(ctx);
    out2[0] = out2[1] = 0;
    if (bytes == 0) return HP_OK;
    HP_TRY(ctx->reward_ws.ensure(256));
    u64 *d = ctx->reward_ws.as<u64>();
    HP_CHECK_HIP(hipMemsetAsync(d, 0, 16, ctx->stream));
    HP_TRY(launch_checksum(dev, bytes, d, ctx->stream, blocks));
    HP_CHECK_HIP(hipMemcpyAsync(out2, d, 16, hipMemcpyDeviceToHost, ctx->stream));
    HP_CHECK_HIP(hipStreamSynchronize(ctx->stream));
    return HP_OK;
}

}  // extern "C"
