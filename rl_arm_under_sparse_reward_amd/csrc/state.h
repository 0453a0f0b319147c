// state.h -- device side of the training state (state.hip): the order of a state's sections, the map between the reference's
// flat named_parameters() order (utils.py:18-27) and the padded parameter arena (agent.h), and the position-weighted checksum.
// Library-internal, not part of the C ABI.
//
// Section order.  ONE function of state.hip, state_layout(agent, buffer, norms, delta, n_episodes, S), writes the table of either
// kind of state -- the 27 small sections, then the buffer --, makes the one offset pass (256-byte boundaries) and returns the size:
//    0 ..  8   actor critic actor_target critic_target adam_actor_m adam_actor_v adam_critic_m adam_critic_v adam_step
//    9 .. 26   o_norm_<field> g_norm_<field> (the eight NORM_FIELDS of each normalizer), rng_key rng_pos
//   full       27 .. 30 buffer_obs buffer_ag buffer_g buffer_actions (n_episodes = current_size), 31 buffer_counters
//   delta      27 buffer_delta_header, 28 buffer_delta_slots, 29 .. 32 buffer_delta_obs buffer_delta_ag buffer_delta_g
//              buffer_delta_actions (room for n_episodes = max_dirty episodes), 33 buffer_counters
// hp_state_layout / hp_state_layout_delta report it; capture, drain, fetch and restore all work from it.
#pragma once
#include "agent.h"

// Sections of a training state, in blob order (hp_state_layout reports name, dtype, count and byte offset of each).
enum {
    ST_ACTOR = 0, ST_CRITIC, ST_ACTOR_TARGET, ST_CRITIC_TARGET,          // float32, flat order
    ST_ADAM_ACTOR_M, ST_ADAM_ACTOR_V, ST_ADAM_CRITIC_M, ST_ADAM_CRITIC_V, // float32, flat order
    ST_ADAM_STEP,                                                        // int64 [1]
    ST_ONORM = 9,                                                        // 8 sections per normalizer, NORM_FIELDS below
    ST_GNORM = 17,
    ST_RNG_KEY = 25, ST_RNG_POS,                                         // uint32 [624], int32 [1]
    ST_BUF_OBS, ST_BUF_AG, ST_BUF_G, ST_BUF_ACT,                         // float64 rows of episodes [0, current_size)
    ST_BUF_COUNTERS,                                                     // int64 [2]: current_size, n_transitions_stored
    ST_SECTIONS = 32
};
// Sections of a DELTA state (hp_state_layout_delta): the small sections ST_ACTOR .. ST_RNG_POS at the same indices, then the buffer
// as the episodes written since a base capture.
enum {
    DS_HEADER = ST_RNG_POS + 1,                                          // int64 [4]: n_dirty, overflow, capture_epoch, since_epoch
    DS_SLOTS,                                                            // int64 [max_dirty]: the dirty slots, ascending
    DS_OBS, DS_AG, DS_G, DS_ACT,                                         // float64 rows of those slots, packed [max_dirty][...]
    DS_COUNTERS,                                                         // int64 [2], as ST_BUF_COUNTERS
    DS_SECTIONS = 34
};
static_assert(DS_COUNTERS + 1 == DS_SECTIONS && DS_SECTIONS == HP_STATE_DELTA_SECTIONS, "delta section count");
#define DS_CHUNK_THREADS 256
#define DS_CHUNK_ITEMS 8
#define DS_CHUNK (DS_CHUNK_THREADS * DS_CHUNK_ITEMS)                     // slots per workgroup of the dirty scan
static_assert(DS_CHUNK == HP_STATE_DIRTY_CHUNK, "rlarm_hip_debug.h names the chunk for the scan's test");
enum { NF_LOCAL_SUM = 0, NF_LOCAL_SUMSQ, NF_LOCAL_COUNT, NF_TOTAL_SUM, NF_TOTAL_SUMSQ, NF_TOTAL_COUNT, NF_MEAN, NF_STD, NORM_FIELDS };
enum { SD_F32 = 0, SD_F64 = 1, SD_I64 = 2, SD_U32 = 3, SD_I32 = 4 };   // hp_state_section::dtype

// one network's flat order -> arena index (pack_net / unpack_net of agent.hip, per element)
struct FlatMap {
    int w1, b1, w2, b2, w3, b3, w4, b4;   // NetLayout offsets
    int K1, H, in1, xdim, act_off, out4;
    int base;                             // first float of the net's segment in the arena (0 / la.total)
    int n;                                // flat elements
};

__host__ __device__ __forceinline__ int flat_to_arena(const FlatMap &m, int j) {
    const int n1 = m.H * m.in1, hh = m.H * m.H;
    if (j < n1) {   // fc1.weight: the critic's action columns sit at act_off in the padded row
        const int r = j / m.in1, c = j - r * m.in1;
        return m.base + m.w1 + r * m.K1 + (c < m.xdim ? c : m.act_off + (c - m.xdim));
    }
    j -= n1;
    if (j < m.H) return m.base + m.b1 + j;
    j -= m.H;
    if (j < hh) return m.base + m.w2 + j;
    j -= hh;
    if (j < m.H) return m.base + m.b2 + j;
    j -= m.H;
    if (j < hh) return m.base + m.w3 + j;
    j -= hh;
    if (j < m.H) return m.base + m.b3 + j;
    j -= m.H;
    if (j < m.out4 * m.H) return m.base + m.w4 + j;
    j -= m.out4 * m.H;
    return m.base + m.b4 + j;
}
