// rng_streams.hip -- an array of device random streams: one legacy MT19937 state per environment of a vectorised simulator.
//
// The reference gives every MPI rank one environment and one numpy stream seeded `seed + rank` (train.py:34-39); n environments
// side by side on one device are n such workers, so stream i is np.random.RandomState(seed_i) -- key[624], pos, has_gauss and
// the cached normal -- and nothing env i draws depends on how many streams stand next to it.  The states are whole MtStates in
// one allocation; the exploring step that consumes them is k_rollout_step_streams (rollout.hip).
#include <vector>

#include "internal.h"

#define RS_SEED_THREADS 64

// numpy _legacy_seeding(int) -> init_genrand for n streams at once: the recurrence is sequential inside a stream and
// independent between streams, so one thread walks one stream.  seeds == nullptr: stream i gets base + i.
__global__ __launch_bounds__(RS_SEED_THREADS) void k_streams_seed(MtState *st, const uint32_t *seeds, uint32_t base, long long n) {
    const long long i = (long long)blockIdx.x * RS_SEED_THREADS + threadIdx.x;
    if (i >= n) return;
    MtState *m = st + i;
    mt_init_genrand(seeds ? seeds[i] : base + (uint32_t)i, m->key);
    m->pos = MT_N;
    m->has_gauss = 0;
    m->gauss = 0.0;
}

// stream-ordered with the kernels that use the states; the pageable side is done with before return
int mt_states_get(hp_rng_streams *s, MtState *host, int64_t first, int64_t count) {
    HP_CHECK_HIP(hipMemcpyAsync(host, s->d_state + first, (size_t)count * sizeof(MtState), hipMemcpyDeviceToHost, s->ctx->stream));
    HP_CHECK_HIP(hipStreamSynchronize(s->ctx->stream));
    return HP_OK;
}

int mt_states_put(hp_rng_streams *s, const MtState *host, int64_t first, int64_t count) {
    HP_CHECK_HIP(hipMemcpyAsync(s->d_state + first, host, (size_t)count * sizeof(MtState), hipMemcpyHostToDevice, s->ctx->stream));
    HP_CHECK_HIP(hipStreamSynchronize(s->ctx->stream));
    return HP_OK;
}

int mt_state_fill(MtState &h, const char *entry, int64_t stream, const uint32_t *key624, int32_t pos, int32_t has_gauss, double gauss) {
    if (pos < 0 || pos > MT_N) {
        if (stream < 0) hp_set_error("%s: pos %d outside [0, 624]", entry, pos);
        else hp_set_error("%s: pos %d of stream %lld outside [0, 624]", entry, pos, (long long)stream);
        return HP_ERR_INVALID;
    }
    memcpy(h.key, key624, sizeof(h.key));
    h.pos = pos;
    h.has_gauss = has_gauss ? 1 : 0;
    h.gauss = has_gauss ? gauss : 0.0;
    return HP_OK;
}

extern "C" {

int hp_streams_create(hp_ctx *ctx, int64_t n, hp_rng_streams **out) {
    HP_REQUIRE(ctx && out, HP_ERR_INVALID, "hp_streams_create: null argument");
    HP_REQUIRE(n > 0 && n < (1 << 24), HP_ERR_INVALID, "hp_streams_create: %lld streams: the count must lie in [1, 2^24)", (long long)n);
    CtxGuard guard(ctx);
    hp_rng_streams *s = new hp_rng_streams();
    s->ctx = ctx;
    s->n = n;
    hipError_t e = hipMalloc((void **)&s->d_state, (size_t)n * sizeof(MtState));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        hp_set_error("hp_streams_create: the states of %lld streams (%zu bytes) cannot be allocated: %s", (long long)n,
                     (size_t)n * sizeof(MtState), hipGetErrorString(e));
        delete s;
        return HP_ERR_HIP;
    }
    int st = hp_streams_seed(s, nullptr, n, 5489u);   // numpy's default key, like a fresh hp_rng
    if (st != HP_OK) {
        (void)hipFree(s->d_state);
        delete s;
        return st;
    }
    *out = s;
    return HP_OK;
}

int hp_streams_seed(hp_rng_streams *s, const uint32_t *seeds_host, int64_t n_seeds, uint32_t base_seed) {
    HP_REQUIRE(s, HP_ERR_INVALID, "hp_streams_seed: null handle");
    HP_SERIALISE(s);
    HP_REQUIRE(n_seeds == s->n, HP_ERR_INVALID, "hp_streams_seed: %lld seeds for %lld streams", (long long)n_seeds, (long long)s->n);
    HP_REQUIRE(seeds_host || (uint64_t)base_seed + (uint64_t)(s->n - 1) <= 0xFFFFFFFFull, HP_ERR_INVALID,
               "Seed must be between 0 and 2**32 - 1");   // numpy's message: base + i would leave the range
    uint32_t *d_seeds = nullptr;
    if (seeds_host) {
        HP_CHECK_HIP(hipMalloc((void **)&d_seeds, (size_t)s->n * 4));
        hipError_t e = hipMemcpyAsync(d_seeds, seeds_host, (size_t)s->n * 4, hipMemcpyHostToDevice, s->ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);
        if (e != hipSuccess) {
            (void)hipFree(d_seeds);
            HP_CHECK_HIP(e);
        }
    }
    const long long blocks = (s->n + RS_SEED_THREADS - 1) / RS_SEED_THREADS;
    hipLaunchKernelGGL(k_streams_seed, dim3((unsigned)blocks), dim3(RS_SEED_THREADS), 0, s->ctx->stream, s->d_state, d_seeds, base_seed,
                       (long long)s->n);
    hipError_t e = hipGetLastError();
    if (d_seeds) {
        if (e == hipSuccess) e = hipStreamSynchronize(s->ctx->stream);   // the list is read by the kernel
        (void)hipFree(d_seeds);
    }
    HP_CHECK_HIP(e);
    return HP_OK;
}

int hp_streams_get_state(hp_rng_streams *s, int64_t i, uint32_t *key624, int32_t *pos, int32_t *has_gauss, double *gauss) {
    HP_REQUIRE(s && key624 && pos && has_gauss && gauss, HP_ERR_INVALID, "hp_streams_get_state: null argument");
    HP_SERIALISE(s);
    HP_REQUIRE(i >= 0 && i < s->n, HP_ERR_INVALID, "hp_streams_get_state: stream %lld outside [0, %lld)", (long long)i, (long long)s->n);
    MtState h;
    HP_TRY(mt_states_get(s, &h, i, 1));
    memcpy(key624, h.key, sizeof(h.key));
    *pos = h.pos;
    *has_gauss = h.has_gauss;
    *gauss = h.gauss;
    return HP_OK;
}

int hp_streams_set_state(hp_rng_streams *s, int64_t i, const uint32_t *key624, int32_t pos, int32_t has_gauss, double gauss) {
    HP_REQUIRE(s && key624, HP_ERR_INVALID, "hp_streams_set_state: null argument");
    HP_SERIALISE(s);
    HP_REQUIRE(i >= 0 && i < s->n, HP_ERR_INVALID, "hp_streams_set_state: stream %lld outside [0, %lld)", (long long)i, (long long)s->n);
    MtState h;
    HP_TRY(mt_state_fill(h, "hp_streams_set_state", -1, key624, pos, has_gauss, gauss));
    return mt_states_put(s, &h, i, 1);
}

int hp_streams_get_all(hp_rng_streams *s, uint32_t *keys, int32_t *pos, int32_t *has_gauss, double *gauss) {
    HP_REQUIRE(s && keys && pos && has_gauss && gauss, HP_ERR_INVALID, "hp_streams_get_all: null argument");
    HP_SERIALISE(s);
    std::vector<MtState> h((size_t)s->n);
    HP_TRY(mt_states_get(s, h.data(), 0, s->n));
    for (int64_t i = 0; i < s->n; ++i) {
        memcpy(keys + i * MT_N, h[i].key, sizeof(h[i].key));
        pos[i] = h[i].pos;
        has_gauss[i] = h[i].has_gauss;
        gauss[i] = h[i].gauss;
    }
    return HP_OK;
}

int hp_streams_set_all(hp_rng_streams *s, const uint32_t *keys, const int32_t *pos, const int32_t *has_gauss, const double *gauss) {
    HP_REQUIRE(s && keys && pos && has_gauss && gauss, HP_ERR_INVALID, "hp_streams_set_all: null argument");
    HP_SERIALISE(s);
    std::vector<MtState> h((size_t)s->n);
    for (int64_t i = 0; i < s->n; ++i) HP_TRY(mt_state_fill(h[i], "hp_streams_set_all", i, keys + i * MT_N, pos[i], has_gauss[i], gauss[i]));
    return mt_states_put(s, h.data(), 0, s->n);
}

void hp_streams_destroy(hp_rng_streams *s) {
    if (!s) return;
    {
        CtxGuard guard(s->ctx);   // the owning device is current and no call on the context is under way while the states go
        if (s->d_state) (void)hipFree(s->d_state);
    }
    delete s;
}

}  // extern "C"
