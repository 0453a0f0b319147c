// Stand-alone check of csrc/stage_block.h on the CPU (built with -fsanitize=address,undefined by tests/test_stage_block_cpu.py): the
// index and size arithmetic of the cycle-opening launch and of the chunked normalizer update, at every episode shape of
// tests/test_gpu_norm.py (multi-chunk table) and tests/test_gpu_cycle_open_direct.py, for 1 .. 5 staged episodes.  Host arrays are
// exactly sized heap memory, so an index past an array or a block is the sanitizer's to find.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stage_block.h"

#define CHECK(cond)                                                                 \
    do {                                                                            \
        if (!(cond)) {                                                              \
            std::fprintf(stderr, "%s:%d: CHECK failed: %s\n", __FILE__, __LINE__, #cond); \
            std::exit(1);                                                           \
        }                                                                           \
    } while (0)

struct Shape {
    int obs, goal, act, T;
    int chunk;      // rows per LDS trip of the normalizer update (0: not part of that table)
    int n_chunks;   // trips over T rows
    int last;       // rows of the last trip
    int trips;      // register trips one episode needs in the direct form (> STORE_DIRECT_CHUNKS: it does not fit)
};

static const Shape SHAPES[] = {
    // the multi-chunk table of tests/test_gpu_norm.py
    {60, 3, 7, 94, 94, 1, 94, 2},
    {60, 3, 7, 95, 94, 2, 1, 2},
    {60, 3, 7, 100, 94, 2, 6, 2},
    {60, 3, 7, 188, 94, 2, 94, 4},
    {130, 5, 6, 100, 44, 3, 12, 4},
    {10, 3, 4, 300, 256, 2, 44, 2},
    {27, 3, 4, 300, 192, 2, 108, 3},
    {256, 256, 1, 30, 11, 3, 8, 6},
    // the cases of tests/test_gpu_cycle_open_direct.py: wide60 and wide130 are rows 3 and 5 above, long300 is row 7
    {152, 3, 4, 100, 0, 0, 0, 4},   // last_fit
    {153, 3, 4, 100, 0, 0, 0, 5},   // first_unfit
    {27, 3, 4, 100, 100, 1, 100, 1},   // n1 .. grow
    {27, 3, 3, 100, 100, 1, 100, 1},   // odd
    {5, 2, 3, 7, 7, 1, 7, 1},          // odd_total
};

static const uint64_t TABLE_LDS = 4 * 624 * 4;   // the draw's four MT19937 rings, which the winners' table reuses (cycle_open.hip)

static void check_norm_chunks(const Shape &s) {
    if (!s.chunk) return;
    size_t lds = 0;
    const int chunk = norm_plan_chunk(s.obs, s.goal, s.T, &lds);
    CHECK(chunk == s.chunk);
    CHECK(lds == (size_t)chunk * (16 + 8 * (size_t)(s.obs + s.goal)) && lds <= 48 * 1024);
    int n = 0, last = 0;
    for (long long r0 = 0; r0 < s.T; r0 += chunk) {   // the loop of norm_update_from_plan_body
        last = (int)((s.T - r0) < chunk ? (s.T - r0) : chunk);
        CHECK(last > 0);
        ++n;
    }
    CHECK(n == s.n_chunks && last == s.last);
}

static void check_block(const Shape &s, int n_new) {
    const long long ep_obs = (long long)(s.T + 1) * s.obs, ep_ag = (long long)(s.T + 1) * s.goal, ep_g = (long long)s.T * s.goal,
                    ep_act = (long long)s.T * s.act;
    const long long ep = ep_obs + ep_ag + ep_g + ep_act;
    const StageBlock L = stage_block_of(n_new, ep_obs, ep_ag, ep_g, ep_act);
    const unsigned nd = L.nd;
    CHECK((long long)nd == n_new * ep && L.n_obs + L.n_ag + L.n_g + (unsigned)(n_new * ep_act) == nd);
    const unsigned nthreads = (unsigned)(STAGE_WG_PER_EPISODE * n_new * STAGE_WG_THREADS);

    // ownership: thread gtid, trip it, half h.  Nothing past nd, nothing twice; everything once exactly when the batch fits
    std::vector<unsigned char> owned(nd, 0);
    std::vector<int> trip_of(nd, -1);
    for (unsigned gtid = 0; gtid < nthreads; ++gtid)
        for (int it = 0; it < STORE_DIRECT_CHUNKS; ++it) {
            const unsigned d = stage_chunk_first(gtid, it, nthreads), m = stage_chunk_doubles(d, nd);
            CHECK(m <= 2u && (d % 2u) == 0u);
            if (m) CHECK(d + m <= nd);
            if (m == 1u) CHECK(d == nd - 1u && (nd & 1u));   // half a chunk: only the last double of an odd block
            if (m == 0u) CHECK(d >= nd);
            for (unsigned h = 0; h < m; ++h) {
                CHECK(owned[d + h] == 0);   // (the vector is nd long: an index past it is the sanitizer's)
                owned[d + h] = 1;
                trip_of[d + h] = it;
            }
        }
    unsigned n_owned = 0;
    for (unsigned d = 0; d < nd; ++d) n_owned += owned[d];
    // the trip a double needs, from the layout alone: chunk d / 2 is trip (d / 2) / nthreads of thread (d / 2) % nthreads
    const unsigned max_trip = ((nd - 1u) / 2u) / nthreads;
    const bool fits = stage_block_direct_fits((uint64_t)ep, n_new, TABLE_LDS);
    CHECK(fits == (max_trip < (unsigned)STORE_DIRECT_CHUNKS));
    CHECK(fits == (n_owned == nd));
    CHECK(fits == (s.trips <= STORE_DIRECT_CHUNKS));
    for (unsigned d = 0; d < nd; ++d)
        if (owned[d]) CHECK((unsigned)trip_of[d] == (d / 2u) / nthreads);
    // trips per episode: the launch has 2 * n_new * 1024 threads, so 2048 chunks per episode and trip whatever n_new is (several
    // odd episodes share their half chunks, which can only save a trip)
    const unsigned ep_trips = (unsigned)(((ep + 1) / 2 + 2047) / 2048);
    CHECK((int)ep_trips == s.trips);
    CHECK(n_new == 1 ? max_trip + 1u == ep_trips : max_trip + 1u <= ep_trips);

    // locate: every double of the block lands where a plain four-array scatter puts it.  Slots: episode e -> (3 e + 1) mod cap,
    // and with three or more staged episodes the last one takes the first one's slot (later wins: the first is dropped)
    const int cap = 7;
    std::vector<long long> slot((size_t)n_new), win((size_t)n_new);
    for (int e = 0; e < n_new; ++e) slot[(size_t)e] = (3 * e + 1) % cap;
    if (n_new >= 3) slot[(size_t)n_new - 1] = slot[0];
    for (int e = 0; e < n_new; ++e) {
        bool dup = false;
        for (int j = e + 1; j < n_new; ++j) dup |= slot[(size_t)j] == slot[(size_t)e];
        win[(size_t)e] = dup ? -1 : slot[(size_t)e];
    }
    std::vector<double> blk(nd);
    for (unsigned d = 0; d < nd; ++d) blk[d] = 1.0 + (double)d;
    const long long len[4] = {ep_obs, ep_ag, ep_g, ep_act};
    const unsigned start[4] = {0u, L.n_obs, L.n_obs + L.n_ag, L.n_obs + L.n_ag + L.n_g};
    // the same block in bytes (buffer.hip's carve and host fill): each array begins where StageBlock says, and copying four exactly
    // sized arrays to those offsets of an exactly sized block gives the block
    const StageBytes nb = stage_bytes_of(n_new, (size_t)ep_obs, (size_t)ep_ag, (size_t)ep_g, (size_t)ep_act);
    const size_t at[4] = {0, nb.at_ag(), nb.at_g(), nb.at_act()}, bytes[4] = {nb.obs, nb.ag, nb.g, nb.act};
    CHECK(nb.total == (size_t)nd * 8 && at[3] + nb.act == nb.total);
    std::vector<char> carved(nb.total);
    for (int a = 0; a < 4; ++a) {
        CHECK(at[a] == (size_t)start[a] * 8 && bytes[a] == (size_t)n_new * (size_t)len[a] * 8);
        const std::vector<double> arr(blk.begin() + start[a], blk.begin() + start[a] + n_new * len[a]);
        std::memcpy(carved.data() + at[a], arr.data(), bytes[a]);
    }
    CHECK(std::memcmp(carved.data(), blk.data(), nb.total) == 0);
    std::vector<double> want[4], got[4];
    for (int a = 0; a < 4; ++a) {
        want[a].assign((size_t)(cap * len[a]), 0.0);
        got[a].assign((size_t)(cap * len[a]), 0.0);
        for (int e = 0; e < n_new; ++e)   // in order: a later episode with the same slot overwrites an earlier one
            std::memcpy(want[a].data() + slot[(size_t)e] * len[a], blk.data() + start[a] + (size_t)e * (size_t)len[a],
                        (size_t)len[a] * sizeof(double));
    }
    for (unsigned d = 0; d < nd; ++d) {
        const StageLoc p = stage_block_locate(L, d);
        CHECK(p.arr < 4u && (long long)p.len == len[p.arr] && p.e < (unsigned)n_new && p.k < p.len);
        CHECK(start[p.arr] + p.e * p.len + p.k == d);
        const long long w = win[p.e];
        if (w >= 0) got[p.arr][(size_t)(w * (long long)p.len + p.k)] = blk[d];
    }
    for (int a = 0; a < 4; ++a) CHECK(std::memcmp(want[a].data(), got[a].data(), want[a].size() * sizeof(double)) == 0);
}

int main() {
    int n_fit = 0, n_unfit = 0;
    for (const Shape &s : SHAPES) {
        check_norm_chunks(s);
        for (int n_new = 1; n_new <= 5; ++n_new) {
            check_block(s, n_new);
            const long long ep = (long long)(s.T + 1) * (s.obs + s.goal) + (long long)s.T * (s.goal + s.act);
            (stage_block_direct_fits((uint64_t)ep, n_new, TABLE_LDS) ? n_fit : n_unfit)++;
        }
    }
    CHECK(n_fit > 0 && n_unfit > 0);
    // the boundary itself: 16384 doubles per episode is the last size that fits, whatever the number of episodes
    for (int n_new = 1; n_new <= 5; ++n_new) {
        CHECK(stage_block_direct_fits(16384, n_new, TABLE_LDS));
        CHECK(!stage_block_direct_fits(16385, n_new, TABLE_LDS));
    }
    // ... unless the winners' table outgrows its LDS, or the block its 32-bit positions
    CHECK(stage_block_direct_fits(100, 624, TABLE_LDS) && !stage_block_direct_fits(100, 625, TABLE_LDS));
    CHECK(!stage_block_direct_fits(1ull << 31, 1, TABLE_LDS));
    // the 256-row cap and the 48 KB budget of the normalizer's chunk, and fewer rows than a chunk
    size_t lds = 0;
    CHECK(norm_plan_chunk(1, 1, 1000, &lds) == 256 && lds == 256 * 32);
    CHECK(norm_plan_chunk(27, 3, 1000, &lds) == 192 && lds == 48 * 1024);
    CHECK(norm_plan_chunk(27, 3, 100, &lds) == 100 && lds == 100 * 256);
    CHECK(norm_plan_chunk(256, 256, 5, &lds) == 5 && lds == 5 * (16 + 4096));
    std::puts("stage_block ok");
    return 0;
}
