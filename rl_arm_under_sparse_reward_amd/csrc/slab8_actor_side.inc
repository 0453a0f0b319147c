// slab8_actor_side.inc -- the actor-side chain of the thin-slab engine: actor -> critic(x, pi(x)) -> Q_pi, actor loss, dX through
// the critic and the actor (ddpg_agent.py:265-277 up to the weight gradients).  Textually included by k_fb_slab8 (slab8.h) and by
// the split launch k_fb_split8 (slab8_split.h), which both declare the names it uses (A, Bk, on, la, lc, ca, ad, H, ring, rbase,
// xin, bufA, bufB, pbuf, dq, rows, dz, w1t, msk, row0, slab, nslab, tid, wave, lane, invB, tl) and the hooks S8_AFTER_CRITIC_FWD / _DX1 / _DX
// and S8_CHAIN_WT, the store policy of this chain's outputs (slab8.h, "store policy": true = write-through, false = ordinary stores
// for outputs only a later launch reads).
    s8_ring_prologue<0, S8_PRO_FIRST>(ring, rbase, on.wf + la.w2);   // (as on the critic side: -0.4 us/update at batch 1024, neutral at 256)
    const PlanRec rec = s8_plan_rec(A.gs, row0);
    float4 wba[6], wbc[6], wh[4], wq[4], wb4[6];
    float w1n[4];
    s8_small_prefetch(on.wf + la.w1, la.K1, wba);
#if S8_NRG == 1   // 4-row slabs: -0.4 us/update at batch 256, -0.2 at 512 k8 (8 rows: +0.2 at 1024, not taken there)
    float ebP[3] = {0.f, 0.f, 0.f}, ebQ[3] = {0.f, 0.f, 0.f};   // biases of the actor trunk and of the critic trunk behind it
    const int ecol_ = 64 * (wave & 3) + lane;
    const bool ekh0_ = S8_BOTH_HALVES || wave < 4;   // (8- / 16-row slabs: both reduction halves run epilogues)
    if (ekh0_) ebP[0] = on.canon[la.b1 + ecol_];
#endif
    __builtin_amdgcn_sched_barrier(0);   // (as on the critic side: what the first layer does not need follows the input loads)
    if (A.gs.plan) s8_gather<S8_CHAIN_WT>(xin, A.gs, rec, 2, row0, A.ldx, A.act_off, ad, A.max_action, A.XP);
    else s8_load(xin, S8_LDX, A.ldx, A.XP + row0 * A.ldx, A.ldx);
    s8_ring_prologue<S8_PRO_FIRST, S8_RING>(ring, rbase, on.wf + la.w2);
    __builtin_amdgcn_sched_barrier(0);
    s8_small_prefetch(on.wf + ca + lc.w1, lc.K1, wbc);
#pragma unroll
    for (int j = 0; j < 4; ++j)
        wh[j] = *reinterpret_cast<const float4 *>(on.canon + la.w4 + (j < ad ? j : ad - 1) * H + 4 * lane);
    wq[0] = *reinterpret_cast<const float4 *>(on.canon + ca + lc.w4 + 4 * lane);
    const float bh = on.canon[la.b4 + (lane < ad ? lane : 0)];
    const float bq = on.canon[ca + lc.b4];
    const float w4c = on.canon[ca + lc.w4 + (tid & 255)];
    {
        const float *w1 = on.canon + ca + lc.w1 + (size_t)(tid & 255) * lc.K1 + A.act_off;
#pragma unroll
        for (int j = 0; j < 4; ++j) w1n[j] = w1[j < ad ? j : ad - 1];
    }
    s8_small_prefetch(on.wd + la.w4, 16, wb4);
#if S8_NRG == 1   // 4-row slabs: -0.4 us/update at batch 256, -0.2 at 512 k8 (8 rows: +0.2 at 1024, not taken there)
    if (ekh0_) {
        ebP[1] = on.canon[la.b2 + ecol_]; ebP[2] = on.canon[la.b3 + ecol_];
        ebQ[0] = on.canon[ca + lc.b1 + ecol_]; ebQ[1] = on.canon[ca + lc.b2 + ecol_]; ebQ[2] = on.canon[ca + lc.b3 + ecol_];
    }
    const float *pP = ebP, *pQ = ebQ;
#else
    const float *pP = nullptr, *pQ = nullptr;
#endif
    __builtin_amdgcn_sched_barrier(0);
    s8_sync();
    s8_trunk<S8_CHAIN_WT>(xin, la, wba, on.wf, on.canon, H, bufA, bufB, pbuf, A.APh1, A.APh2, A.APh3, row0, ring, rbase, on.wf + ca + lc.w2,
             tl, 1, msk[2], msk[3], msk[4], pP);
    S8_TSTAMP(tl, 5);
    float u_mine[S8_RPW], th_mine[S8_RPW];
#pragma unroll
    for (int i = 0; i < S8_RPW; ++i) {   // actor head: tanh -> action block of the critic input (models.py:24, :38); lane j owns output j
        const int rr = wave + S8_WAVES * i;
        u_mine[i] = th_mine[i] = 0.f;
        const float z = s8_rowdots(bufA, S8_LD, rr < S8_ROWS ? rr : 0, ad, wh);
        if (lane < ad && rr < S8_ROWS) {
            th_mine[i] = tanhf(z + bh);
            u_mine[i] = (A.max_action * th_mine[i]) / A.max_action;
            xin[rr * S8_LDX + A.act_off + lane] = u_mine[i];
            A.XP[(row0 + rr) * A.ldx + A.act_off + lane] = u_mine[i];
            A.TP[(row0 + rr) * 16 + lane] = th_mine[i];
        }
    }
    S8_TSTAMP(tl, 6);
    s8_sync();
    S8_TSTAMP(tl, 7);
    s8_trunk(xin, lc, wbc, on.wf + ca, on.canon + ca, H, bufA, bufB, pbuf, nullptr, nullptr, nullptr, row0, ring, rbase,
             on.wd + ca + lc.w3, tl, 8, msk[0], msk[1], nullptr, pQ);
    {
#pragma unroll
        for (int i = 0; i < S8_RPW; ++i) {
            const int rr = wave + S8_WAVES * i;
            const float q = s8_rowdots(bufA, S8_LD, rr < S8_ROWS ? rr : 0, 1, wq);
            if (lane == 0 && rr < S8_ROWS) {
                rows[1][rr] = q + bq;
                A.QP[(row0 + rr) * 16] = q + bq;
            }
        }
    }
    if (tid < 256) {
#pragma unroll
        for (int j = 0; j < 4; ++j) w1t[j * 256 + tid] = w1n[j];
    }
    s8_sync();
    S8_TSTAMP(tl, 13);
    S8_AFTER_CRITIC_FWD;   // (split launch: the critic's forward fragments and head rows are not read again)
    // ---- actor loss (ddpg_agent.py:265-267)
    float keep_q = 0.f, keep_u = 0.f;
    if (tid < S8_ROWS) {   // (four lanes of wave 0, beside the head's backward step below: nothing here feeds it any more)
        const size_t m = row0 + tid;
        const bool live = (int)m < Bk.B;
        float u4[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) u4[j] = xin[tid * S8_LDX + A.act_off + j];   // (all four asked for at once; columns past ad are padding)
        float sq = live ? rows[1][tid] : 0.f, su = 0.f;
        if (live) {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < ad) su += u4[j] * u4[j];
        }
        sq = s8_rows_sum_to_lane0(sq);
        su = s8_rows_sum_to_lane0(su);
        keep_q = sq;
        keep_u = su;
    }
    // dQ_pi / dq of a live row is -1 / B (the mean's gradient, ddpg_agent.py:265): known without a trip through the LDS, so the head's
    // backward step no longer waits behind a barrier for four lanes to write it
    s8_head_bwd_inplace_rows(-invB, (int)row0, Bk.B, w4c, bufA);   // bufA holds h3 of critic(x, pi(x))
    s8_sync();
    S8_TSTAMP(tl, 14);
#ifdef SLAB_TIMELINE   // per-wave stamps of this layer (A.tl + 128: entry, products done, merge barrier passed, layer's closing barrier passed)
    unsigned long long *wtl_ = (tl && tl != A.tl) ? A.tl + 128 : nullptr;
    s8_big_layer(bufA, S8_LD, ring, rbase, on.wd + ca + lc.w3, on.wd + ca + lc.w2, SE_MASK, nullptr, 0, pbuf, bufB, S8_LD, msk[1],
                 nullptr, nullptr, 0, nullptr, nullptr, wtl_);
    s8_sync();
    S8_WSTAMP(wtl_, 24);
#else
    s8_big_layer(bufA, S8_LD, ring, rbase, on.wd + ca + lc.w3, on.wd + ca + lc.w2, SE_MASK, nullptr, 0, pbuf, bufB, S8_LD, msk[1]);
    s8_sync();
#endif
    S8_TSTAMP(tl, 15);
    S8_AFTER_CRITIC_DX1;   // (split launch: the dX fragments of the critic's third layer are not read again)
    s8_big_layer(bufB, S8_LD, ring, rbase, on.wd + ca + lc.w2, on.wd + la.w3, SE_MASK, nullptr, 0, pbuf, bufA, S8_LD, msk[0]);
    s8_sync();
    S8_TSTAMP(tl, 16);
    S8_AFTER_CRITIC_DX;   // (split launch: this chain reads no critic parameter from here on)
    {   // d L / d(action block of the critic input), then through the L2 penalty and tanh; lane j owns action j
        float4 w1g[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) w1g[j] = *reinterpret_cast<const float4 *>(w1t + j * 256 + 4 * lane);
#pragma unroll
        for (int i = 0; i < S8_RPW; ++i) {
            const int rr = wave + S8_WAVES * i;
            const float sj = s8_rowdots(bufA, S8_LD, rr < S8_ROWS ? rr : 0, ad, w1g);
            if (lane < 16 && rr < S8_ROWS) {
                const size_t m = row0 + rr;
                float v = 0.f;
                if (lane < ad && (int)m < Bk.B) {
                    const float gu = Bk.action_l2 * (2.f * u_mine[i] / (float)(Bk.B * ad)) + sj;
                    const float gt = (gu / A.max_action) * A.max_action;
                    v = gt * (1.f - th_mine[i] * th_mine[i]);
                }
                dz[rr * 20 + lane] = v;
                out_store<S8_CHAIN_WT>(Bk.dZ + m * 16 + lane, v);
            }
        }
    }
    s8_sync();
    S8_TSTAMP(tl, 17);
    s8_small_layer<S8_CHAIN_WT>(dz, 20, 16, wb4, SE_MASK, nullptr, 0, pbuf, bufB, S8_LD, msk[4], nullptr, Bk.dK3 + row0 * H);
    s8_sync();
    S8_TSTAMP(tl, 18);
    s8_big_layer<S8_CHAIN_WT>(bufB, S8_LD, ring, rbase, on.wd + la.w3, on.wd + la.w2, SE_MASK, nullptr, 0, pbuf, bufA, S8_LD, msk[3], nullptr,
                 nullptr, 0, Bk.dK2 + row0 * H);
    s8_sync();
    S8_TSTAMP(tl, 19);
    s8_big_layer<S8_CHAIN_WT>(bufA, S8_LD, ring, rbase, on.wd + la.w2, nullptr, SE_MASK, nullptr, 0, pbuf, bufB, S8_LD, msk[2], nullptr,
                 nullptr, 0, Bk.dK1 + row0 * H);
    // The end of the chain.  Nothing below reads the LDS or another wave's registers: the loss partials are in thread 0's registers
    // since the actor loss above, so they need no barrier.  With ordinary stores nothing waits for publication either -- no drain, no
    // barrier: each wave ends behind its own last store and the kernel-end release publishes them.  What stays: the barrier of the
    // time-line build (stamp 20 = EVERY wave has issued its dK1 stores), and the write-through instantiation as it was (A/B).
    if (S8_CHAIN_WT || S8_TL_BUILD) s8_sync();
    S8_TSTAMP(tl, 20);
    if (tid == 0) {
        out_store<S8_CHAIN_WT>(Bk.part + nslab + slab, keep_q);
        out_store<S8_CHAIN_WT>(Bk.part + 2 * nslab + slab, keep_u);
    }
    S8_TSTAMP(tl, 21);
