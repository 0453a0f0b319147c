// store_device.h -- device side of replay_buffer.store_episode's scatter (replay_buffer.py:39-42), shared by buffer.hip's
// k_store_scatter and the cycle-opening kernel (cycle_open.hip).
#pragma once
#include "internal.h"
#include "stage_block.h"

// Episode i of the staged batch goes to slot slots[i] unless a LATER staged episode has the same slot (numpy's
// `buffers[idxs] = mb` lets the last occurrence win).  One of `parts` workgroups per episode copies a strided share of its
// values.  Workgroup-uniform control flow; `slot_of(j)` reads slots[j] (plain or agent-scope load, the caller knows).
// Every (episode, part) also stamps its slot with the buffer's capture epoch, READ FROM DEVICE MEMORY so that a cached graph keeps
// stamping right after a capture advanced it (state.hip: delta states).  A dropped episode stamps too: its slot was written, by
// the winner, with the same value.
template <class SlotOf>
__device__ __forceinline__ void store_scatter_share(SlotOf slot_of, long long i, int part, int parts, long long n_new,
                                                    const double *s_obs, const double *s_ag, const double *s_g,
                                                    const double *s_act, double *obs, double *ag, double *g, double *act,
                                                    long long ep_obs, long long ep_ag, long long ep_g, long long ep_act,
                                                    uint32_t *slot_epoch, const uint32_t *epoch) {
    const long long slot = slot_of(i);
    if (threadIdx.x == 0) slot_epoch[slot] = *epoch;
    int dup = 0;
    for (long long j = i + 1 + threadIdx.x; j < n_new; j += blockDim.x) dup |= (slot_of(j) == slot);
    if (__syncthreads_or(dup)) return;
    const long long t0 = (long long)part * blockDim.x + threadIdx.x, step = (long long)parts * blockDim.x;
    for (long long k = t0; k < ep_obs; k += step) obs[slot * ep_obs + k] = s_obs[i * ep_obs + k];
    for (long long k = t0; k < ep_ag; k += step) ag[slot * ep_ag + k] = s_ag[i * ep_ag + k];
    for (long long k = t0; k < ep_g; k += step) g[slot * ep_g + k] = s_g[i * ep_g + k];
    for (long long k = t0; k < ep_act; k += step) act[slot * ep_act + k] = s_act[i * ep_act + k];
}

// ---- the direct form of the cycle-opening kernel: the staged batch still lies in a pinned HOST block (hp_buffer::ring), laid out
// obs | ag | g | actions back to back like the device staging, `nd` doubles in all.  The block is cut into 16-byte chunks, chunk c
// belonging to thread c mod `nthreads` of the scatter workgroups together; a thread holds at most STORE_DIRECT_CHUNKS of them in
// registers (cycle_open_direct_fits).  The block's base is page aligned, so every chunk load is; only the LAST chunk of a block
// with an odd number of doubles is half a chunk, loaded as 8 bytes -- nothing is read past the block.  Which chunk is whose, what
// of it lies in the block and where a double of the block goes: stage_block.h (StageBlock, STORE_DIRECT_CHUNKS).

// all of a thread's loads, issued back to back before anything waits for them (one PCIe round trip)
__device__ __forceinline__ void stage_block_load(const double *__restrict__ blk, unsigned nd, unsigned gtid, unsigned nthreads,
                                                 double (&v)[STORE_DIRECT_CHUNKS][2]) {
#pragma unroll
    for (int it = 0; it < STORE_DIRECT_CHUNKS; ++it) {
        const unsigned d = stage_chunk_first(gtid, it, nthreads), m = stage_chunk_doubles(d, nd);
        v[it][0] = v[it][1] = 0.0;
        if (m == 2u) {
            const double2 x = *reinterpret_cast<const double2 *>(blk + d);
            v[it][0] = x.x;
            v[it][1] = x.y;
        } else if (m == 1u) {
            v[it][0] = blk[d];
        }
    }
}

// the same chunks into the device staging (same layout), as write-through stores: the normalizer workgroup of the SAME launch
// reads them behind a counter
__device__ __forceinline__ void stage_block_put(double *stage, unsigned nd, unsigned gtid, unsigned nthreads,
                                                const double (&v)[STORE_DIRECT_CHUNKS][2]) {
#pragma unroll
    for (int it = 0; it < STORE_DIRECT_CHUNKS; ++it) {
        const unsigned d = stage_chunk_first(gtid, it, nthreads), m = stage_chunk_doubles(d, nd);
#pragma unroll
        for (int h = 0; h < 2; ++h)
            if ((unsigned)h < m)
                __hip_atomic_store(reinterpret_cast<long long *>(stage) + d + h, __double_as_longlong(v[it][h]), __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ... and into the buffer rows of their episodes' slots.  win[e]: the slot of staged episode e, or -1 where a later staged episode
// has the same slot (the rule at the top of this file).
__device__ __forceinline__ void stage_block_scatter(const StageBlock &L, const long long *win, unsigned gtid, unsigned nthreads,
                                                    const double (&v)[STORE_DIRECT_CHUNKS][2], double *obs, double *ag, double *g,
                                                    double *act) {
#pragma unroll
    for (int it = 0; it < STORE_DIRECT_CHUNKS; ++it) {
        const unsigned d = stage_chunk_first(gtid, it, nthreads), m = stage_chunk_doubles(d, L.nd);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if ((unsigned)h >= m) continue;
            const StageLoc p = stage_block_locate(L, d + (unsigned)h);
            double *arr = p.arr == 0u ? obs : p.arr == 1u ? ag : p.arr == 2u ? g : act;
            const long long slot = win[p.e];
            if (slot >= 0) arr[slot * (long long)p.len + p.k] = v[it][h];
        }
    }
}
