// stage_ring.h -- host bookkeeping of the pinned ring that k_cycle_open reads a cycle's fresh episodes from (cycle_open.hip).
// Plain C++: the event and allocation calls go through `Api`, so the rotation, growth and release rules run on the CPU under a
// sanitizer with a stub (tests/host/stage_ring_main.cpp); buffer.hip supplies the HIP one.
//
// N blocks of pinned, device-mapped host memory, one fence each.  A cycle takes the next block (acquire), the host fills it, the
// launch that reads it is enqueued, and the block's fence is recorded BEHIND that launch (mark).  acquire waits for the fence of the
// block it hands out, so the host never overwrites episodes that a queued launch has not read.  All blocks have one size; a larger
// need waits for every pending fence, frees all blocks and allocates them anew (`moved`: their addresses changed, so whatever
// baked an address in -- a captured graph -- is stale).
//
// Api:  using Event, Stream;  int alloc(size_t bytes, void **host, void **dev);  void free_block(void *host);
//       int event_create(Event *);  int event_sync(Event);  int event_record(Event, Stream);  void event_destroy(Event);
// (int results: 0 = success, anything else is returned to the caller as it is.)
#pragma once
#include <cstddef>

template <class Api, int N = 3> struct StageRing {
    static_assert(N >= 2, "one block being read by the device, one being filled by the host");
    static constexpr int SLOTS = N;
    struct Slot {
        void *host = nullptr, *dev = nullptr;
        typename Api::Event fence{};
        bool has_fence = false, pending = false;
    };
    Slot slot[N];
    size_t bytes = 0;   // of every block
    int next = 0;

    // the block of the next cycle, at least `need` bytes, free to overwrite.  *moved: the blocks were (re)allocated.
    int acquire(Api &api, size_t need, int *idx, bool *moved) {
        *moved = false;
        if (need > bytes) {
            if (int st = drain(api)) return st;
            free_blocks(api);
            for (int i = 0; i < N; ++i)
                if (int st = api.alloc(need, &slot[i].host, &slot[i].dev)) {
                    free_blocks(api);
                    return st;
                }
            bytes = need;
            next = 0;
            *moved = true;
        }
        Slot &s = slot[next];
        if (s.pending) {
            if (int st = api.event_sync(s.fence)) return st;
            s.pending = false;
        }
        *idx = next;
        next = (next + 1) % N;
        return 0;
    }

    // behind the launch that reads block idx
    int mark(Api &api, int idx, typename Api::Stream stream) {
        Slot &s = slot[idx];
        if (!s.has_fence) {
            if (int st = api.event_create(&s.fence)) return st;
            s.has_fence = true;
        }
        if (int st = api.event_record(s.fence, stream)) return st;
        s.pending = true;
        return 0;
    }

    void release(Api &api) {
        (void)drain(api);
        free_blocks(api);
        for (Slot &s : slot) {
            if (s.has_fence) api.event_destroy(s.fence);
            s.has_fence = false;
            s.pending = false;
        }
        next = 0;
    }

private:
    int drain(Api &api) {   // every launch that reads a block has finished
        int first = 0;
        for (Slot &s : slot) {
            if (!s.pending) continue;
            const int st = api.event_sync(s.fence);
            if (st && !first) first = st;
            s.pending = false;
        }
        return first;
    }
    void free_blocks(Api &api) {
        for (Slot &s : slot) {
            if (s.host) api.free_block(s.host);
            s.host = s.dev = nullptr;
        }
        bytes = 0;
    }
};
