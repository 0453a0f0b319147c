// stage_block.h -- the index and size arithmetic of the cycle-opening launch (cycle_open.hip) and of the chunked normalizer update
// (norm_device.h), with no loads or stores: which doubles of a staged block a scatter thread owns, where a double of the block
// goes, whether a batch fits the direct form, how many plan rows one LDS trip of the normalizer takes, and the byte carve of a
// staged batch (buffer.hip).  Plain C++ for host and device, so all of it runs on the CPU under a sanitizer
// (tests/host/stage_block_main.cpp); store_device.h, norm_device.h, norm.hip, cycle_open.hip and buffer.hip call it.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__)
#define STAGE_HD __host__ __device__ __forceinline__
#else
#define STAGE_HD inline
#endif

// ---- a staged batch in bytes (buffer.hip): the float64 arrays obs | ag | g | actions of n_new episodes back to back, on the device
// (st_obs .. st_act) and in every host block that is copied there
struct StageBytes {
    size_t obs, ag, g, act, total;
    size_t at_ag() const { return obs; }              // where each array after the first begins
    size_t at_g() const { return obs + ag; }
    size_t at_act() const { return obs + ag + g; }
};
inline StageBytes stage_bytes_of(long long n_new, size_t ep_obs, size_t ep_ag, size_t ep_g, size_t ep_act) {
    StageBytes n;
    n.obs = (size_t)n_new * ep_obs * 8;
    n.ag = (size_t)n_new * ep_ag * 8;
    n.g = (size_t)n_new * ep_g * 8;
    n.act = (size_t)n_new * ep_act * 8;
    n.total = n.obs + n.ag + n.g + n.act;
    return n;
}

// ---- the direct form: the staged batch lies in a pinned HOST block, obs | ag | g | actions back to back, `nd` doubles in all
// (store_device.h).  The block is cut into 16-byte chunks, chunk c belonging to thread c mod `nthreads` of the scatter workgroups
// together, as that thread's trip c / nthreads; a thread holds at most STORE_DIRECT_CHUNKS trips in registers.
#define STORE_DIRECT_CHUNKS 4
#define STAGE_WG_THREADS 1024    // threads of a scatter workgroup (OPEN_THREADS)
#define STAGE_WG_PER_EPISODE 2   // scatter workgroups per staged episode (OPEN_PARTS)

struct StageBlock {   // the four arrays of a staged batch as one run of doubles
    unsigned n_obs, n_ag, n_g;           // doubles of the first three arrays (n_new episodes each)
    unsigned ep_obs, ep_ag, ep_g, ep_act;
    unsigned nd;
};

// the block of `inc` staged episodes of ep_* doubles each (the caller knows that it fits: stage_block_direct_fits)
STAGE_HD StageBlock stage_block_of(long long inc, long long ep_obs, long long ep_ag, long long ep_g, long long ep_act) {
    StageBlock L;
    L.n_obs = (unsigned)(inc * ep_obs);
    L.n_ag = (unsigned)(inc * ep_ag);
    L.n_g = (unsigned)(inc * ep_g);
    L.ep_obs = (unsigned)ep_obs;
    L.ep_ag = (unsigned)ep_ag;
    L.ep_g = (unsigned)ep_g;
    L.ep_act = (unsigned)ep_act;
    L.nd = (unsigned)(inc * (ep_obs + ep_ag + ep_g + ep_act));
    return L;
}

// first double of the chunk that thread `gtid` of `nthreads` owns in trip `it`; its two halves are d and d + 1
STAGE_HD unsigned stage_chunk_first(unsigned gtid, int it, unsigned nthreads) { return 2u * (gtid + (unsigned)it * nthreads); }

// how many doubles of the chunk at `d` lie in a block of `nd`: 2, 1 (the LAST chunk of a block with an odd number of doubles)
// or 0 (the thread has nothing in this trip)
STAGE_HD unsigned stage_chunk_doubles(unsigned d, unsigned nd) { return d + 1u < nd ? 2u : (d < nd ? 1u : 0u); }

struct StageLoc {
    unsigned arr;   // 0 obs, 1 ag, 2 g, 3 actions
    unsigned e, k;  // staged episode, offset in its row
    unsigned len;   // doubles of one episode's row of that array: the double goes to arr[slot * len + k]
};

// position d < L.nd of the block -> array, staged episode, offset
STAGE_HD StageLoc stage_block_locate(const StageBlock &L, unsigned d) {
    StageLoc o;
    unsigned r = d;
    if (r < L.n_obs) { o.arr = 0u; o.len = L.ep_obs; }
    else if ((r -= L.n_obs) < L.n_ag) { o.arr = 1u; o.len = L.ep_ag; }
    else if ((r -= L.n_ag) < L.n_g) { o.arr = 2u; o.len = L.ep_g; }
    else { r -= L.n_g; o.arr = 3u; o.len = L.ep_act; }
    o.e = r / o.len;
    o.k = r - o.e * o.len;
    return o;
}

// Can the scatter workgroups take `n_new` staged episodes of `ep_doubles` each from the pinned block themselves?  Every thread
// keeps its chunks in registers across the wait for the slots, and the winners' table (two long long per staged episode) lies in
// the launch's LDS, of which `table_lds_bytes` are there for it.
STAGE_HD bool stage_block_direct_fits(uint64_t ep_doubles, int64_t n_new, uint64_t table_lds_bytes) {
    const uint64_t nd = (uint64_t)n_new * ep_doubles;
    const uint64_t threads = (uint64_t)STAGE_WG_PER_EPISODE * n_new * STAGE_WG_THREADS;
    return nd < (1ull << 31) && (nd + 1) / 2 <= STORE_DIRECT_CHUNKS * threads &&
           (uint64_t)n_new * 2 * sizeof(long long) <= table_lds_bytes;
}

// ---- the normalizer update from a plan (norm_device.h): LDS rows per chunk of norm_update_from_plan_body and the bytes they
// take -- what 48 KB of LDS hold (plan record + one float64 per column and row), at most 256
#define NORM_PLAN_REC_BYTES 16   // sizeof(PlanRec)
STAGE_HD int norm_plan_chunk(int obs_dim, int goal_dim, long long rows, size_t *lds_bytes) {
    const int W = obs_dim + goal_dim;
    int chunk = (int)((48 * 1024) / ((size_t)NORM_PLAN_REC_BYTES + (size_t)W * 8));
    chunk = chunk > 256 ? 256 : chunk;
    chunk = rows < chunk ? (int)rows : chunk;
    *lds_bytes = (size_t)chunk * ((size_t)NORM_PLAN_REC_BYTES + (size_t)W * 8);
    return chunk;
}
