// Stand-alone check of csrc/stage_ring.h on the CPU (built with -fsanitize=address,undefined by tests/test_stage_ring_cpu.py):
// rotation, the wait before a block is handed out again, growth, failures of the allocator and release, with a stub in place of
// the event and allocation calls.  The stub models the device as a queue of launches: a recorded event "fires" only when the test
// says the device got that far, and event_sync lets the device run up to it.  Blocks are ordinary heap memory, so a use after
// free or a write past a block is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "stage_ring.h"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

struct StubApi {
    struct Ev {
        long recorded_at = -1;   // position in the device queue behind which the event lies (-1: never recorded)
    };
    using Event = Ev *;
    using Stream = int;
    long enqueued = 0, done = 0;          // launches enqueued / finished by the device
    int live_blocks = 0, live_events = 0, syncs = 0, allocs = 0;
    int fail_alloc_at = -1;               // the n-th alloc from now fails (0 = the next one)
    std::set<void *> blocks;

    int alloc(size_t bytes, void **host, void **dev) {
        *host = *dev = nullptr;
        if (fail_alloc_at == 0) {
            fail_alloc_at = -1;
            return 7;
        }
        if (fail_alloc_at > 0) --fail_alloc_at;
        *host = std::malloc(bytes);
        CHECK(*host);
        *dev = *host;
        blocks.insert(*host);
        ++live_blocks;
        ++allocs;
        return 0;
    }
    void free_block(void *host) {
        CHECK(blocks.erase(host) == 1);
        std::free(host);
        --live_blocks;
    }
    int event_create(Event *e) {
        *e = new Ev();
        ++live_events;
        return 0;
    }
    int event_sync(Event e) {
        CHECK(e && e->recorded_at >= 0);
        ++syncs;
        if (done < e->recorded_at) done = e->recorded_at;   // the host waited: the device got that far
        return 0;
    }
    int event_record(Event e, Stream) {
        e->recorded_at = enqueued;
        return 0;
    }
    void event_destroy(Event e) {
        delete e;
        --live_events;
    }
};

// one cycle as hp_agent_train_cycle runs it: acquire, fill, enqueue the launch that reads the block, mark.  Launch: the block a
// queued launch reads and the byte it must find there.
struct Launch {
    const unsigned char *block;
    size_t bytes;
    unsigned char fill;
};

template <int N> static void cycle(StageRing<StubApi, N> &ring, StubApi &api, std::vector<Launch> &queue, size_t bytes, unsigned char fill,
                                   bool *moved_out = nullptr) {
    int idx = -1;
    bool moved = false;
    CHECK(ring.acquire(api, bytes, &idx, &moved) == 0);
    CHECK(idx >= 0 && idx < N && ring.bytes >= bytes);
    // no launch that the device has not finished may still read this block
    for (long i = api.done; i < api.enqueued; ++i) CHECK(queue[(size_t)i].block != ring.slot[idx].host);
    std::memset(ring.slot[idx].host, fill, bytes);
    queue.push_back({static_cast<const unsigned char *>(ring.slot[idx].dev), bytes, fill});
    ++api.enqueued;
    CHECK(ring.mark(api, idx, 0) == 0);
    if (moved_out) *moved_out = moved;
}

template <int N> static void run() {
    StubApi api;
    StageRing<StubApi, N> ring;
    std::vector<Launch> queue;
    bool moved = false;
    // rotation with the device far behind: the first N cycles never wait, every later one waits for the launch N cycles back
    cycle(ring, api, queue, 100, 1, &moved);
    CHECK(moved && api.live_blocks == N && api.syncs == 0);
    for (int i = 1; i < N; ++i) {
        cycle(ring, api, queue, 100, (unsigned char)(1 + i), &moved);
        CHECK(!moved && api.syncs == 0);
    }
    CHECK(api.done == 0);
    for (int i = 0; i < 3 * N; ++i) {   // the ring wraps three times
        const long before = api.enqueued;
        cycle(ring, api, queue, 100, (unsigned char)(10 + i), &moved);
        CHECK(!moved && api.done == before - N + 1);   // waited exactly for the launch that read this block, no further
    }
    // the device catches up: the last N launches find their blocks as the host left them
    for (long i = api.enqueued - N; i < api.enqueued; ++i)
        for (size_t k = 0; k < queue[(size_t)i].bytes; ++k) CHECK(queue[(size_t)i].block[k] == queue[(size_t)i].fill);
    api.done = api.enqueued;
    // a block whose launch already finished is handed out without a second wait on a fired fence doing harm
    const int syncs0 = api.syncs;
    cycle(ring, api, queue, 60, 77, &moved);   // smaller need: no re-allocation
    CHECK(!moved && ring.bytes == 100 && api.syncs == syncs0 + 1);
    // growth: waits for EVERY pending launch, then all blocks move
    cycle(ring, api, queue, 100, 78);
    const long pending_to = api.enqueued;
    const int allocs0 = api.allocs;
    cycle(ring, api, queue, 4096, 79, &moved);
    CHECK(moved && ring.bytes == 4096 && api.allocs == allocs0 + N && api.live_blocks == N && api.done >= pending_to);
    cycle(ring, api, queue, 4096, 80, &moved);
    CHECK(!moved);
    // the allocator fails in the middle of a growth: nothing leaks, the ring is empty and usable again
    api.fail_alloc_at = 1;
    int idx = -1;
    CHECK(ring.acquire(api, 10000, &idx, &moved) == 7);
    CHECK(api.live_blocks == 0 && ring.bytes == 0);
    cycle(ring, api, queue, 10000, 81, &moved);
    CHECK(moved && api.live_blocks == N);
    // an acquire that is never marked (the launch failed): the block is simply handed out again later
    CHECK(ring.acquire(api, 10, &idx, &moved) == 0 && !moved);
    for (int i = 0; i < 2 * N; ++i) cycle(ring, api, queue, 10000, (unsigned char)(90 + i));
    // release with launches still queued: waits for them, frees everything, and may be called twice
    ring.release(api);
    CHECK(api.live_blocks == 0 && api.live_events == 0 && api.done == api.enqueued);
    ring.release(api);
    CHECK(api.live_blocks == 0 && api.live_events == 0);
    // ... and the ring can start over
    cycle(ring, api, queue, 32, 5, &moved);
    CHECK(moved);
    ring.release(api);
    CHECK(api.live_blocks == 0 && api.live_events == 0);
}

int main() {
    run<2>();
    run<3>();
    run<4>();
    std::puts("stage_ring ok");
    return 0;
}
