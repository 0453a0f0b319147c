// mt19937_wave.h -- numpy's remaining legacy draws on the device stream: randn, uniform(low, high), binomial(1, p).
//
// These are the three draws of ddpg_agent._select_actions (:174-184).  Their word consumption is data dependent twice over --
// the polar method rejects pairs, and a cached second normal carries from one randn call into the next -- and the draws of one
// environment are only a few dozen words, so the walk is made by ONE wave on the LDS ring of mt19937_device.h.  The wave is a
// 64-thread workgroup of its own or one wave of a wider workgroup that runs one walk per wave, each on its own ring: the lane is
// the lane inside the wavefront and every barrier below is wave-local (mt_tid<64>, mt_barrier<64>):
//   * all lanes hold the same cursor / cached normal: control flow is wave-uniform, nothing is exchanged between lanes but
//     ballots and one shuffle;
//   * randn: lane k evaluates the polar attempt at cursor + 4 k (an attempt always consumes two doubles, accepted or not); a
//     ballot ranks the accepted attempts, the first `need` of them are taken, and the lane of the last one taken moves the cursor.
//     The logarithms of the attempts taken are computed side by side instead of one after the other;
//   * every float64 operation that decides a word count (2u - 1, r2, the comparisons, the inversion loop of the binomial) is an
//     explicit IEEE operation, so the stream position cannot drift from numpy's.  Only log() may differ from glibc's, in the last
//     place of a VALUE.
// The cached normal lives in MtState (has_gauss, gauss) next to (key, pos): numpy's whole legacy state is device resident.
#pragma once
#include "mt19937_device.h"

#define MW_THREADS 64

__device__ __forceinline__ int mw_lane() { return mt_tid<MW_THREADS>(); }
__device__ __forceinline__ void mw_sync() { mt_barrier<MW_THREADS>(); }

// The one-wave walk: an MtWg of MW_THREADS threads + numpy's cached second normal.  Constructing one (or load()) is mt_load and
// store() is mt_store: both are cooperative across the wave, so both run under wave-uniform control flow only.
struct MwState {
    MtWg g;
    int has_gauss;
    double gauss;
    __device__ __forceinline__ MwState() : has_gauss(0), gauss(0.0) {}
    __device__ __forceinline__ MwState(const MtState *st, uint32_t (*ring)[MT_N]) { load(st, ring); }
    __device__ __forceinline__ void load(const MtState *st, uint32_t (*ring)[MT_N]) {
        has_gauss = st->has_gauss;
        gauss = st->gauss;
        mt_load<MW_THREADS>(g, st, ring, nullptr);
    }
    __device__ __forceinline__ void store(MtState *st) const { mt_store<MW_THREADS>(g, st, has_gauss, &gauss); }
};

__device__ __forceinline__ double mw_double_at(const MtWg &g, long long abs) {
    return mt_to_double(mt_word(g, abs), mt_word(g, abs + 1));
}

// legacy_gauss (numpy/random/src/legacy/legacy-distributions.c) `count` times: emit(i, z) is called once per value, by whichever
// lane computed it.  A pending cached normal is value 0; an odd remainder leaves its second normal cached.
template <class Emit>
__device__ __forceinline__ void mw_draw_normal(MwState &w, long long count, Emit emit) {
    const int lane = mw_lane();
    long long done = 0;
    if (count > 0 && w.has_gauss) {
        if (lane == 0) emit(0, w.gauss);
        w.has_gauss = 0;
        w.gauss = 0.0;
        done = 1;
    }
    while (done < count) {
        const long long need = (count - done + 1) / 2;   // accepted attempts still to take
        mt_ensure<MW_THREADS>(w.g, w.g.cursor + 4 * MW_THREADS);
        const long long at = w.g.cursor + 4 * lane;
        const double x1 = __dsub_rn(__dmul_rn(2.0, mw_double_at(w.g, at)), 1.0);
        const double x2 = __dsub_rn(__dmul_rn(2.0, mw_double_at(w.g, at + 2)), 1.0);
        const double r2 = __dadd_rn(__dmul_rn(x1, x1), __dmul_rn(x2, x2));
        const bool acc = (r2 < 1.0) && (r2 != 0.0);
        const unsigned long long m = __ballot(acc);
        const int total = __popcll(m);
        const int rank = __popcll(m & ((1ull << lane) - 1ull));
        const long long take = total < need ? (long long)total : need;
        double fx1 = 0.0;
        if (acc && rank < take) {
            const double f = __dsqrt_rn(__ddiv_rn(__dmul_rn(-2.0, log(r2)), r2));
            fx1 = __dmul_rn(f, x1);
            const long long i = done + 2 * rank;
            emit(i, __dmul_rn(f, x2));
            if (i + 1 < count) emit(i + 1, fx1);
        }
        if (total >= need) {
            const int last = __ffsll((long long)__ballot(acc && rank == need - 1)) - 1;   // lane of the last attempt taken
            if (done + 2 * need > count) {   // its second normal is the one numpy caches
                w.gauss = __shfl(fx1, last);
                w.has_gauss = 1;
            }
            w.g.cursor += 4 * (last + 1);
            done = count;
        } else {
            w.g.cursor += 4 * MW_THREADS;
            done += 2 * take;
        }
    }
}

// random_uniform(low, range) = low + range * next_double, `count` times (count <= MW_THREADS per call: one value per lane)
template <class Emit>
__device__ __forceinline__ void mw_draw_uniform(MwState &w, double low, double range, int count, Emit emit) {
    mt_ensure<MW_THREADS>(w.g, w.g.cursor + 2 * count);
    const int lane = mw_lane();
    if (lane < count) emit(lane, __dadd_rn(low, __dmul_rn(range, mw_double_at(w.g, w.g.cursor + 2 * lane))));
    w.g.cursor += 2 * count;
}

// legacy binomial(1, eps): legacy_random_binomial_original -> random_binomial_inversion(n = 1, p) with p = eps for eps <= 0.5 and
// 1 - that of p = 1 - eps otherwise.  qn = exp(1 * log(1 - p)) comes from the host (glibc, once).  The loop is the reference's,
// whole: bound = min(n, np + 10 sqrt(npq + 1)) is 1 for n = 1, so X = 2 redraws.  Every lane computes the same thing.
__device__ __forceinline__ int mw_draw_binomial1(MwState &w, double eps, double qn) {
    const bool reflect = !(eps <= 0.5);
    const double p = reflect ? __dsub_rn(1.0, eps) : eps;
    const double q = __dsub_rn(1.0, p);
    const long long bound = 1;
    long long X = 0;
    double px = qn;
    mt_ensure<MW_THREADS>(w.g, w.g.cursor + 2);
    double U = mw_double_at(w.g, w.g.cursor);
    w.g.cursor += 2;
    while (U > px) {
        X += 1;
        if (X > bound) {
            X = 0;
            px = qn;
            mt_ensure<MW_THREADS>(w.g, w.g.cursor + 2);
            U = mw_double_at(w.g, w.g.cursor);
            w.g.cursor += 2;
        } else {
            U = __dsub_rn(U, px);
            px = __ddiv_rn(__dmul_rn(__dmul_rn((double)(1 - X + 1), p), px), __dmul_rn((double)X, q));
        }
    }
    return reflect ? (int)(1 - X) : (int)X;
}
