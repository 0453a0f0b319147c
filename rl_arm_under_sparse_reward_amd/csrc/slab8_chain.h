// slab8_chain.h -- segments of the thin-slab chains that more than one chain body runs, one definition each (included by slab8.h
// inside namespace S8_NS, once per slab height, in front of the chain bodies).
//   s8_critic_loss   the critic-side chain of fb_slab8_body (slab8.h) and the C chain of fb_split8_body (slab8_split.h)
// A segment takes the caller's thread index and leaves the predicate that selects its threads to the caller: with either inside the
// segment the update kernels no longer compile to the listing they had (profiles/chain_segments_refactor.txt).

// Critic loss of a slab (ddpg_agent.py:255-263) from the per-row scalars in the LDS (rows: Q' | Q | reward).  Called by the threads
// tid < S8_ROWS, thread r for row r: dL/dQ of the row into keep_g, and in thread 0 the slab's sum of squared TD errors into keep_a.
__device__ __forceinline__ void s8_critic_loss(int tid, const float (*rows)[S8_ROWS], size_t row0, const BwdSlabArgs &Bk, float invB,
                                               float &keep_g, float &keep_a) {
    const size_t m = row0 + tid;
    float g = 0.f, sq = 0.f;
    if ((int)m < Bk.B) {
        float y = rows[2][tid] + Bk.gamma * rows[0][tid];
        y = fminf(fmaxf(y, -Bk.clip_ret), 0.f);
        const float d = y - rows[1][tid];
        sq = d * d;
        g = -2.f * d * invB;
    }
    sq = s8_rows_sum_to_lane0(sq);
    keep_g = g;
    keep_a = sq;
}
