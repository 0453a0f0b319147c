// rng_parallel.hip -- the reference's random stream entered at many offsets at once: hp_rng_advance (skip n words) and the
// parallel form of the sampler's index draw (her.py:24-33) behind hp_rng_set_parallel.
//
// The sequential draw (mt19937_device.h) is ONE workgroup walking the stream; at 2^18 transitions that walk is 97 % of a
// sample_device call.  MT19937 is linear over GF(2) (mt19937_jump.h), so the raw block at any stream offset J is an XOR of
// windows of the next 19937 + 623 generated words, selected by the coefficients of x^J mod phi.  One call of the parallel draw:
//   k_mt_window    1 workgroup    the 33 raw blocks behind the loaded key -> `win` (only when more than one segment is needed)
//   k_mt_jumpfill  P workgroups   segment p: jump to generated block p * 16 (window in LDS, lane k accumulates word k; the
//                                 coefficient bits are wave-uniform and walked on the scalar side), then twist the segment's
//                                 other 15 blocks; RAW words go to `raw` (block 0 = the loaded key), tempering happens on read
//   k_par_count / k_par_emit      randint(N), then randint(T): accept flags of the masked rejection over a window of the
//                                 stream behind the cursor, chunk counts, the i-th accepted word goes to index i; the
//                                 position behind the B-th accepted word is the next cursor
//   k_par_uniform                 the 2 B + 2 B words of the two uniform draws at fixed offsets from there; workgroup 0
//                                 commits: final (key, pos) in numpy's representation, straight out of `raw`
//   k_draw_plan_tail              the sequential draw, which returns at once when the commit happened
// How many words a batch consumes is data dependent.  The windows are sized for the WORST acceptance (just above 1/2, N or
// T = 2^k + 1): each rejection draw may look at R = 2 B + m words, m = 10 ceil(sqrt(2 B)) + 100.  It fails when fewer than
// B of R words are accepted; with acceptance >= 1/2, Hoeffding gives P <= exp(-2 (R/2 - B)^2 / R) = exp(-m^2 / (2 R))
// <= exp(-50) < 2^-72 per draw, 2^-71 for the two.  A failed draw is handled all the same, without a host round trip:
// nothing is committed (d_state untouched, ctl->done stays 0) and k_draw_plan_tail does the whole draw sequentially.
#include "mt19937_device.h"
#include "mt19937_jump.h"

#include <chrono>

#define MTP_SEG_BLOCKS 16                       // blocks per segment: one jump per 16 blocks of twisting
#define MTP_SEG_WORDS (MTP_SEG_BLOCKS * MT_N)
#define MTP_WIN_BLOCKS 33                       // 33 * 624 = 20592 >= 19937 + 623
#define MTP_WIN_WORDS (MTP_WIN_BLOCKS * MT_N)
#define MTP_JUMP_THREADS 640                    // 10 waves: lanes 0 .. 623 own one word of the target block each
#define MTP_MAX_SEGMENTS 4096                   // ~5 M transitions per call; larger draws stay sequential
#define MTP_PRESET_SEGMENTS 256                 // table built by hp_rng_set_parallel: draws up to 2^18 need no further host work
#define MTP_THREADS 256
#define MTP_ITEMS 8
#define MTP_CHUNK (MTP_THREADS * MTP_ITEMS)     // candidate words per workgroup of a rejection pass
#define MTP_LDS_BYTES ((4 * MT_N + MTP_WIN_WORDS) * 4)   // twist ring + window: 92352 bytes of the CU's 160 KB

struct ParCtl {
    long long c[3];      // cursor (word index into `raw`) in front of randint(N), randint(T), the uniform draws
    int fail[2];         // rejection draw 0 / 1 ran out of window: nothing is committed.  One flag per draw, each written by
                         // that draw's k_par_emit and read by LATER launches only (a flag read and written inside one launch
                         // could split a workgroup in front of a barrier)
    int done;            // the commit happened: k_draw_plan_tail has nothing to do
    long long n_parallel, n_fallback;
};

// ------------------------------------------------------------------------------- kernels
__global__ __launch_bounds__(MT_THREADS) void k_mt_window(const MtState *st, uint32_t *win) {
    __shared__ uint32_t ring[4][MT_N];
    MtWg g;
    mt_load(g, st, ring, nullptr);
    for (int j = 0; j < MTP_WIN_BLOCKS; ++j) {
        mt_generate_block(g);
        const uint32_t *blk = ring[(g.nblk - 1) & 3];
        for (int k = threadIdx.x; k < MT_N; k += MT_THREADS) win[j * MT_N + k] = blk[k];
    }
}

// z_{J + k} = XOR over the set coefficients c_i of g_J of z_{k + i}: `w` = the window in LDS, `coef` = g_J (312 limbs,
// the same for every lane: read and walked as scalars, zero limbs skipped)
__device__ __forceinline__ uint32_t mt_jump_word(const uint32_t *w, const uint64_t *coef, int k) {
    uint32_t acc = 0;
    for (int l = 0; l < MTJ_LIMBS; ++l) {
        const uint64_t v = coef[l];
        uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
        const uint32_t *base = w + k + l * 64;
        while (lo) {
            acc ^= base[__builtin_ctz(lo)];
            lo &= lo - 1u;
        }
        base += 32;
        while (hi) {
            acc ^= base[__builtin_ctz(hi)];
            hi &= hi - 1u;
        }
    }
    return acc;
}

__device__ __forceinline__ void mt_window_to_lds(const uint32_t *win, uint32_t *w) {
    const uint4 *src = reinterpret_cast<const uint4 *>(win);
    uint4 *dst = reinterpret_cast<uint4 *>(w);
    for (int i = threadIdx.x; i < MTP_WIN_WORDS / 4; i += blockDim.x) dst[i] = src[i];
    __syncthreads();
}

// segment p of the raw stream: generated blocks [p * 16, p * 16 + 16) below n_gen; raw block 1 + j = generated block j
__global__ __launch_bounds__(MTP_JUMP_THREADS) void k_mt_jumpfill(const MtState *st, const uint32_t *win, const uint64_t *table,
                                                                   uint32_t *raw, int n_gen, ParCtl *ctl) {
    extern __shared__ uint32_t smem[];
    uint32_t(*ring)[MT_N] = reinterpret_cast<uint32_t(*)[MT_N]>(smem);
    uint32_t *w = smem + 4 * MT_N;
    const int p = blockIdx.x, tid = threadIdx.x;
    MtWg g;   // p > 0: ring block 0 is the block the segment's jump lands on
    g.blk = ring;
    g.nblk = 1;
    int next, end = (p + 1) * MTP_SEG_BLOCKS;
    if (end > n_gen) end = n_gen;
    if (p == 0) {
        mt_load<MTP_JUMP_THREADS>(g, st, ring, nullptr);
        if (tid < MT_N) raw[tid] = ring[0][tid];
        if (tid == 0) {
            ctl->c[0] = g.cursor;
            ctl->fail[0] = ctl->fail[1] = 0;
            ctl->done = 0;
        }
        next = 0;
    } else {
        mt_window_to_lds(win, w);
        next = p * MTP_SEG_BLOCKS;
        if (tid < MT_N) raw[(size_t)(1 + next) * MT_N + tid] = ring[0][tid] = mt_jump_word(w, table + (size_t)(p - 1) * MTJ_LIMBS, tid);
        next += 1;
    }
    __syncthreads();
    for (int j = next; j < end; ++j) {
        mt_generate_block<MTP_JUMP_THREADS>(g);
        if (tid < MT_N) raw[(size_t)(1 + j) * MT_N + tid] = ring[(g.nblk - 1) & 3][tid];
    }
}

// hp_rng_advance: the block `coef` jumps to becomes the key
__global__ __launch_bounds__(MTP_JUMP_THREADS) void k_mt_jump_state(const uint32_t *win, const uint64_t *coef, MtState *st, int pos) {
    extern __shared__ uint32_t smem[];
    mt_window_to_lds(win, smem);
    if (threadIdx.x < MT_N) st->key[threadIdx.x] = mt_jump_word(smem, coef, threadIdx.x);
    if (threadIdx.x == 0) st->pos = pos;
}

struct RejectPass {      // one masked-rejection draw of `batch` values in [0, rng] as device-wide passes
    const uint32_t *raw;
    long long w_end;     // words of `raw` that may be used
    long long window;    // R: candidate words this draw may look at
    long long batch;
    const BufMeta *meta; // rng = meta->current_size - 1 when non-null (randint(N)), else high - 1
    long long high;
    int which;           // 0: e (cursor c[0] -> c[1]), 1: t (c[1] -> c[2])
};
__device__ __forceinline__ uint32_t rp_rng(const RejectPass &a) { return (uint32_t)((a.meta ? a.meta->current_size : a.high) - 1); }

// candidate `it` of this thread: word index it * 256 + tid of the workgroup's chunk (coalesced); accepted value in v
__device__ __forceinline__ bool rp_candidate(const RejectPass &a, long long start, uint32_t rng, uint32_t mask, int it, uint32_t &v,
                                             long long &pos) {
    const long long idx = (long long)blockIdx.x * MTP_CHUNK + it * MTP_THREADS + threadIdx.x;
    pos = start + idx;
    if (idx >= a.window || pos >= a.w_end) return false;
    v = mt_temper(a.raw[pos]) & mask;
    return v <= rng;
}

__global__ __launch_bounds__(MTP_THREADS) void k_par_count(RejectPass a, const ParCtl *ctl, int *counts) {
    __shared__ int wave_n[MTP_THREADS / 64];
    const uint32_t rng = rp_rng(a);
    if ((a.which && ctl->fail[0]) || rng == 0u) return;     // (rng == 0: numpy consumes nothing, k_par_emit reads no counts)
    const uint32_t mask = mt_bound_mask(rng);
    const long long start = ctl->c[a.which];
    int n = 0;
#pragma unroll
    for (int it = 0; it < MTP_ITEMS; ++it) {
        uint32_t v;
        long long pos;
        n += __popcll(__ballot(rp_candidate(a, start, rng, mask, it, v, pos)));
    }
    if ((threadIdx.x & 63) == 0) wave_n[threadIdx.x >> 6] = n;
    __syncthreads();
    if (threadIdx.x == 0) counts[blockIdx.x] = wave_n[0] + wave_n[1] + wave_n[2] + wave_n[3];
}

__global__ __launch_bounds__(MTP_THREADS) void k_par_emit(RejectPass a, ParCtl *ctl, const int *counts, int n_chunks, PlanRec *plan) {
    __shared__ long long red[2][MTP_THREADS / 64];
    __shared__ int wave_n[MTP_ITEMS][MTP_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t rng = rp_rng(a);
    if (a.which && ctl->fail[0]) return;
    const long long start = ctl->c[a.which];
    if (rng == 0u) {
        for (long long i = (long long)blockIdx.x * MTP_THREADS + tid; i < a.batch; i += (long long)gridDim.x * MTP_THREADS)
            (&plan[i].e)[a.which] = 0;
        if (blockIdx.x == 0 && tid == 0) ctl->c[a.which + 1] = start;
        return;
    }
    // accepted words in the chunks in front of this one, and in all of them
    long long before = 0, total = 0;
    for (int j = tid; j < n_chunks; j += MTP_THREADS) {
        const int c = counts[j];
        total += c;
        if (j < (int)blockIdx.x) before += c;
    }
    for (int o = 32; o > 0; o >>= 1) {
        before += __shfl_down(before, o);
        total += __shfl_down(total, o);
    }
    if (lane == 0) {
        red[0][wave] = before;
        red[1][wave] = total;
    }
    __syncthreads();
    before = red[0][0] + red[0][1] + red[0][2] + red[0][3];
    total = red[1][0] + red[1][1] + red[1][2] + red[1][3];
    if (total < a.batch) {      // the window held fewer than B accepted words: fall back
        if (blockIdx.x == 0 && tid == 0) ctl->fail[a.which] = 1;
        return;
    }
    if (before >= a.batch) return;
    const uint32_t mask = mt_bound_mask(rng);
    uint32_t v[MTP_ITEMS];
    long long pos[MTP_ITEMS];
    int within[MTP_ITEMS];
    bool acc[MTP_ITEMS];
#pragma unroll
    for (int it = 0; it < MTP_ITEMS; ++it) {
        acc[it] = rp_candidate(a, start, rng, mask, it, v[it], pos[it]);
        const unsigned long long m = __ballot(acc[it]);
        within[it] = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_n[it][wave] = __popcll(m);
    }
    __syncthreads();
    long long rank = before;
#pragma unroll
    for (int it = 0; it < MTP_ITEMS; ++it) {
        long long mine = rank;
#pragma unroll
        for (int wv = 0; wv < MTP_THREADS / 64; ++wv) {
            const int c = wave_n[it][wv];
            mine += (wv < wave) ? c : 0;
            rank += c;
        }
        mine += within[it];
        if (acc[it] && mine < a.batch) {
            (&plan[mine].e)[a.which] = (int)v[it];
            if (mine == a.batch - 1) ctl->c[a.which + 1] = pos[it] + 1;
        }
    }
}

__global__ __launch_bounds__(MTP_THREADS) void k_par_uniform(ParCtl *ctl, const uint32_t *raw, long long w_end, long long batch, int T,
                                                            double future_p, PlanRec *plan, MtState *st) {
    if (ctl->fail[0] || ctl->fail[1]) return;
    const long long c = ctl->c[2], end = c + 4 * batch;
    if (end > w_end) return;       // cannot happen with the window the launcher sized; a shrunk one (debug hook) falls back
    auto u = [&](long long at) { return mt_to_double(mt_temper(raw[at]), mt_temper(raw[at + 1])); };
    for (long long i = (long long)blockIdx.x * MTP_THREADS + threadIdx.x; i < batch; i += (long long)gridDim.x * MTP_THREADS) {
        PlanRec r = plan[i];
        r.her = mt_her_flag(u(c + 2 * i), future_p);
        r.fut = mt_her_future(r.t, T, u(c + 2 * batch + 2 * i));
        plan[i] = r;
    }
    if (blockIdx.x == 0) {         // commit: the final state in numpy's representation
        mt_commit<MTP_THREADS>(st, end, [&](long long b) { return raw + (size_t)b * MT_N; });
        if (threadIdx.x == 0) {
            ctl->done = 1;
            ctl->n_parallel += 1;
        }
    }
}

// always enqueued behind the parallel kernels: nothing to do after a commit, the whole draw otherwise
__global__ __launch_bounds__(MT_THREADS) void k_draw_plan_tail(ParCtl *ctl, MtState *st, const BufMeta *meta, int T, long long batch,
                                                              double future_p, PlanRec *plan) {
    __shared__ uint32_t ring[4][MT_N];
    __shared__ int ibuf[MT_IBUF];
    if (ctl->done) return;
    mt_her_plan(st, meta->current_size, T, batch, 1, future_p, plan, ring, ibuf);
    if (threadIdx.x == 0) ctl->n_fallback += 1;
}

// ------------------------------------------------------------------------------ host side
static int par_lds_attr() {
    static const hipError_t e = [] {
        hipError_t a = hipFuncSetAttribute(reinterpret_cast<const void *>(k_mt_jumpfill), hipFuncAttributeMaxDynamicSharedMemorySize, MTP_LDS_BYTES);
        if (a != hipSuccess) return a;
        return hipFuncSetAttribute(reinterpret_cast<const void *>(k_mt_jump_state), hipFuncAttributeMaxDynamicSharedMemorySize, MTP_WIN_WORDS * 4);
    }();
    HP_CHECK_HIP(e);
    return HP_OK;
}

static bool stream_capturing(hipStream_t s) {
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) {
        (void)hipGetLastError();
        return true;
    }
    return cs != hipStreamCaptureStatusNone;
}

// the segment table g_{p S}, p = 1 .. n, S = 16 blocks: one multiplication by g_S each.  Allocates and uploads: not under capture.
static int par_table_ensure(hp_rng *rng, int n) {
    const int have = (int)(rng->par_polys.size() / MTJ_LIMBS);
    if (n <= have) return HP_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const mtj::Phi &f = mtj::phi();
    HP_REQUIRE(f.ok, HP_ERR_STATE, "MT19937's characteristic polynomial could not be derived (Berlekamp-Massey self-check failed)");
    rng->par_polys.resize((size_t)n * MTJ_LIMBS);
    MtPoly step, cur, nxt;
    if (have == 0) {
        mtj::jump_poly(MTP_SEG_WORDS, step);
        memcpy(rng->par_polys.data(), step.w, sizeof(step.w));
    } else {
        memcpy(step.w, rng->par_polys.data(), sizeof(step.w));
    }
    const int from = have ? have : 1;
    memcpy(cur.w, rng->par_polys.data() + (size_t)(from - 1) * MTJ_LIMBS, sizeof(cur.w));
    for (int p = from; p < n; ++p) {
        mtj::mulmod(cur, step, f, nxt);
        cur = nxt;
        memcpy(rng->par_polys.data() + (size_t)p * MTJ_LIMBS, cur.w, sizeof(cur.w));
    }
    rng->par_table_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    hipStream_t s = rng->ctx->stream;
    HP_CHECK_HIP(hipStreamSynchronize(s));     // earlier draws may still read the table that is about to be freed
    HP_TRY(rng->par_table.ensure(rng->par_polys.size() * 8));
    HP_CHECK_HIP(hipMemcpyAsync(rng->par_table.p, rng->par_polys.data(), rng->par_polys.size() * 8, hipMemcpyHostToDevice, s));
    HP_CHECK_HIP(hipStreamSynchronize(s));
    return HP_OK;
}

static int par_ctl_ensure(hp_rng *rng) {
    if (rng->d_par) return HP_OK;
    HP_CHECK_HIP(hipMalloc((void **)&rng->d_par, sizeof(ParCtl)));
    HP_CHECK_HIP(hipMemsetAsync(rng->d_par, 0, sizeof(ParCtl), rng->ctx->stream));
    HP_CHECK_HIP(hipStreamSynchronize(rng->ctx->stream));
    return HP_OK;
}

void rng_parallel_release(hp_rng *rng) {
    if (rng->d_par) (void)hipFree(rng->d_par);
    rng->d_par = nullptr;
    rng->par_raw.release();
    rng->par_win.release();
    rng->par_counts.release();
    rng->par_table.release();
    rng->par_poly.release();
}

int rng_launch_plan_sample(hp_rng *rng, const BufMeta *d_meta, int32_t T, int64_t batch, double future_p, PlanRec *d_plan) {
    if (rng->par_min_batch <= 0 || batch < rng->par_min_batch) return rng_launch_plan(rng, d_meta, 0, T, batch, 1, future_p, d_plan);
    hipStream_t s = rng->ctx->stream;
    // window of one rejection draw and of the whole call (header comment): block 0 = the loaded key, then n_gen generated blocks
    const long long margin = 10 * (long long)ceil(sqrt(2.0 * (double)batch)) + 100;
    const long long window = 2 * batch + margin;
    const long long words = MT_N + 2 * window + 4 * batch;
    const long long n_gen = (words + MT_N - 1) / MT_N;       // (one block more than `words` needs: block 0 is counted in it)
    const long long segments = (n_gen + MTP_SEG_BLOCKS - 1) / MTP_SEG_BLOCKS;
    const long long n_chunks = (window + MTP_CHUNK - 1) / MTP_CHUNK;
    const size_t raw_bytes = (size_t)(1 + n_gen) * MT_N * 4, win_bytes = (size_t)MTP_WIN_WORDS * 4, cnt_bytes = (size_t)n_chunks * 4;
    const bool grow = raw_bytes > rng->par_raw.bytes || win_bytes > rng->par_win.bytes || cnt_bytes > rng->par_counts.bytes ||
                      (size_t)(segments - 1) * MTJ_LIMBS > rng->par_polys.size();
    // a draw too large for the table, or one that would have to allocate inside a stream capture, stays sequential: same result
    if (segments > MTP_MAX_SEGMENTS || (grow && stream_capturing(s))) return rng_launch_plan(rng, d_meta, 0, T, batch, 1, future_p, d_plan);
    if (grow) {
        HP_CHECK_HIP(hipStreamSynchronize(s));      // earlier asynchronous draws may still use the scratch about to be freed
        HP_TRY(rng->par_raw.ensure(raw_bytes));
        HP_TRY(rng->par_win.ensure(win_bytes));
        HP_TRY(rng->par_counts.ensure(cnt_bytes));
        HP_TRY(par_table_ensure(rng, (int)segments - 1));
    }
    HP_TRY(par_lds_attr());
    long long w_end = (1 + n_gen) * MT_N;
    if (rng->par_debug_window > 0) {
        if (rng->par_debug_window < w_end) w_end = rng->par_debug_window;
        rng->par_debug_window = 0;
    }
    uint32_t *raw = rng->par_raw.as<uint32_t>(), *win = rng->par_win.as<uint32_t>();
    int *counts = rng->par_counts.as<int>();
    ParCtl *ctl = rng->d_par;
    if (segments > 1) hipLaunchKernelGGL(k_mt_window, dim3(1), dim3(MT_THREADS), 0, s, rng->d_state, win);
    hipLaunchKernelGGL(k_mt_jumpfill, dim3((unsigned)segments), dim3(MTP_JUMP_THREADS), MTP_LDS_BYTES, s, rng->d_state, win,
                       rng->par_table.as<uint64_t>(), raw, (int)n_gen, ctl);
    RejectPass a{raw, w_end, window, (long long)batch, d_meta, 0, 0};
    hipLaunchKernelGGL(k_par_count, dim3((unsigned)n_chunks), dim3(MTP_THREADS), 0, s, a, ctl, counts);
    hipLaunchKernelGGL(k_par_emit, dim3((unsigned)n_chunks), dim3(MTP_THREADS), 0, s, a, ctl, counts, (int)n_chunks, d_plan);
    RejectPass t{raw, w_end, window, (long long)batch, nullptr, (long long)T, 1};
    hipLaunchKernelGGL(k_par_count, dim3((unsigned)n_chunks), dim3(MTP_THREADS), 0, s, t, ctl, counts);
    hipLaunchKernelGGL(k_par_emit, dim3((unsigned)n_chunks), dim3(MTP_THREADS), 0, s, t, ctl, counts, (int)n_chunks, d_plan);
    const long long u_wgs = (batch + MTP_THREADS - 1) / MTP_THREADS, cap = (long long)rng->ctx->cu_count * 8;
    hipLaunchKernelGGL(k_par_uniform, dim3((unsigned)(u_wgs < cap ? u_wgs : cap)), dim3(MTP_THREADS), 0, s, ctl, raw, w_end,
                       (long long)batch, (int)T, future_p, d_plan, rng->d_state);
    hipLaunchKernelGGL(k_draw_plan_tail, dim3(1), dim3(MT_THREADS), 0, s, ctl, rng->d_state, d_meta, (int)T, (long long)batch, future_p, d_plan);
    HP_CHECK_HIP(hipGetLastError());
    return HP_OK;
}

// --------------------------------------------------------------------------------- C ABI
extern "C" {

int hp_mt_jump_poly(uint64_t n_words, uint64_t *limbs312) {
    HP_REQUIRE(limbs312, HP_ERR_INVALID, "hp_mt_jump_poly: null argument");
    MtPoly g;
    HP_REQUIRE(mtj::jump_poly(n_words, g), HP_ERR_STATE,
               "MT19937's characteristic polynomial could not be derived (Berlekamp-Massey self-check failed)");
    memcpy(limbs312, g.w, sizeof(g.w));
    return HP_OK;
}

// skip n_words 32-bit words as if drawn and thrown away (RandomState.bytes(4 n)): pos arithmetic inside the loaded key, a jump
// to the block the cursor ends in otherwise
int hp_rng_advance(hp_rng *rng, uint64_t n_words) {
    HP_REQUIRE(rng, HP_ERR_INVALID, "hp_rng_advance: null handle");
    HP_REQUIRE(n_words < (1ull << 62), HP_ERR_INVALID, "hp_rng_advance: n_words must be below 2^62");
    HP_SERIALISE(rng);
    if (n_words == 0) return HP_OK;
    hipStream_t s = rng->ctx->stream;
    int32_t pos = 0;
    HP_CHECK_HIP(hipMemcpyAsync(&pos, &rng->d_state->pos, 4, hipMemcpyDeviceToHost, s));
    HP_CHECK_HIP(hipStreamSynchronize(s));
    long long b;          // cursor in words, block 0 = the loaded key
    int new_pos;
    mt_final_block((long long)pos + (long long)n_words, b, new_pos);
    if (b == 0) {
        HP_CHECK_HIP(hipMemcpyAsync(&rng->d_state->pos, &new_pos, 4, hipMemcpyHostToDevice, s));
        HP_CHECK_HIP(hipStreamSynchronize(s));
        return HP_OK;
    }
    MtPoly g;     // generated block b - 1 starts (b - 1) * 624 words behind z_0
    HP_REQUIRE(mtj::jump_poly((uint64_t)(b - 1) * MT_N, g), HP_ERR_STATE,
               "MT19937's characteristic polynomial could not be derived (Berlekamp-Massey self-check failed)");
    HP_TRY(rng->par_win.ensure((size_t)MTP_WIN_WORDS * 4));
    HP_TRY(rng->par_poly.ensure(sizeof(g.w)));
    HP_TRY(par_lds_attr());
    HP_CHECK_HIP(hipMemcpyAsync(rng->par_poly.p, g.w, sizeof(g.w), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(k_mt_window, dim3(1), dim3(MT_THREADS), 0, s, rng->d_state, rng->par_win.as<uint32_t>());
    hipLaunchKernelGGL(k_mt_jump_state, dim3(1), dim3(MTP_JUMP_THREADS), MTP_WIN_WORDS * 4, s, rng->par_win.as<uint32_t>(),
                       rng->par_poly.as<uint64_t>(), rng->d_state, (int)new_pos);
    HP_CHECK_HIP(hipGetLastError());
    HP_CHECK_HIP(hipStreamSynchronize(s));     // `g` is pageable host memory
    return HP_OK;
}

int hp_rng_set_parallel(hp_rng *rng, int64_t min_batch) {
    HP_REQUIRE(rng, HP_ERR_INVALID, "hp_rng_set_parallel: null handle");
    HP_SERIALISE(rng);
    if (min_batch <= 0) {
        rng->par_min_batch = 0;
        return HP_OK;
    }
    HP_REQUIRE(!stream_capturing(rng->ctx->stream), HP_ERR_STATE, "hp_rng_set_parallel: not inside a stream capture");
    HP_TRY(par_ctl_ensure(rng));
    HP_TRY(par_table_ensure(rng, MTP_PRESET_SEGMENTS - 1));
    rng->par_min_batch = min_batch;
    return HP_OK;
}

int hp_rng_parallel_info(hp_rng *rng, int64_t *min_batch, int64_t *n_parallel, int64_t *n_fallback) {
    HP_REQUIRE(rng, HP_ERR_INVALID, "hp_rng_parallel_info: null handle");
    HP_SERIALISE(rng);
    ParCtl h;
    memset(&h, 0, sizeof(h));
    if (rng->d_par) {
        HP_CHECK_HIP(hipMemcpyAsync(&h, rng->d_par, sizeof(h), hipMemcpyDeviceToHost, rng->ctx->stream));
        HP_CHECK_HIP(hipStreamSynchronize(rng->ctx->stream));
    }
    if (min_batch) *min_batch = rng->par_min_batch;
    if (n_parallel) *n_parallel = h.n_parallel;
    if (n_fallback) *n_fallback = h.n_fallback;
    return HP_OK;
}

int hp_rng_debug_set_window(hp_rng *rng, int64_t words) {
    HP_REQUIRE(rng && words >= 0, HP_ERR_INVALID, "hp_rng_debug_set_window: bad argument");
    HP_SERIALISE(rng);
    rng->par_debug_window = words;
    return HP_OK;
}

int hp_rng_debug_table_ms(hp_rng *rng, double *ms) {
    HP_REQUIRE(rng && ms, HP_ERR_INVALID, "hp_rng_debug_table_ms: null argument");
    *ms = rng->par_table_ms;
    return HP_OK;
}

}  // extern "C"
