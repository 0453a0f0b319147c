// mt19937_jump.h -- jump polynomials of MT19937 on the host (host code only, no device needed).
//
// MT19937 is linear over GF(2): with phi the characteristic polynomial of its one-word transition (degree 19937), every bit
// of the sequence of GENERATED raw (untempered) words z_n obeys  XOR_{i : phi_i} z_{n+i} = 0, and for g_J(x) = x^J mod phi(x)
//     z_{n+J} = XOR over the set coefficients c_i of g_J of z_{n+i},   i < 19937
// (Haramoto, Matsumoto, Nishimura, Panneton, L'Ecuyer 2008: "Efficient jump ahead for F2-linear random number generators").
// The seed words of a stream are NOT generated words (init_genrand fills 31 bits of key[0] that the recurrence never reads),
// so z_0 is the first word of the block AFTER a loaded key.
//
// phi is not written down here: it is recovered once per process by Berlekamp-Massey from 2 x 19937 bits of the generator's
// own output (bit 0 of consecutive raw words of seed 5489) and checked -- degree 19937, and it annihilates every bit of a
// second, independently seeded sequence -- before anything uses it.  Polynomials are 312 limbs of 64 bits, bit i of limb
// i / 64 = coefficient of x^i.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#include "internal.h"   // mt_init_genrand

#define MTJ_DEG 19937
#define MTJ_LIMBS 312                       // 312 * 64 = 19968 > 19937: holds phi itself too
#define MTJ_TOP (MTJ_DEG & 63)              // bit of limb 311 that is x^19937

struct MtPoly { uint64_t w[MTJ_LIMBS]; };

namespace mtj {

// raw (untempered) generated words of numpy's init_genrand(seed): z_0 .. z_{n-1}, z_0 = first word after the seed block
inline std::vector<uint32_t> raw_words(uint32_t seed, size_t n) {
    std::vector<uint32_t> s(624 + n);
    mt_init_genrand(seed, s.data());
    for (size_t k = 624; k < s.size(); ++k) {
        const uint32_t y = (s[k - 624] & 0x80000000u) | (s[k - 623] & 0x7fffffffu);
        s[k] = s[k - 624 + 397] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
    }
    return std::vector<uint32_t>(s.begin() + 624, s.end());
}

struct Phi {
    bool ok = false;
    MtPoly p{};                 // the full polynomial, bit 19937 set
    std::vector<int> low;       // exponents of its terms below x^19937
};

// Berlekamp-Massey over GF(2) on bit-packed sequences: the connection polynomial C (C_0 = 1) of s_0 .. s_{n-1} with
// s_j = XOR_{i=1..L} C_i s_{j-i}; the characteristic polynomial is its reciprocal x^L C(1/x).
inline Phi derive_phi() {
    Phi out;
    const int n = 2 * MTJ_DEG;
    const std::vector<uint32_t> z = raw_words(5489u, n);
    // r = the sequence reversed (r_j = s_{n-1-j}), so that the discrepancy at step t, XOR_i C_i s_{t-i}, is the parity of
    // C AND (r shifted down by n-1-t): consecutive bits on both sides
    const int RL = (n + 63) / 64 + MTJ_LIMBS + 2;
    std::vector<uint64_t> r(RL, 0);
    for (int j = 0; j < n; ++j)
        if (z[n - 1 - j] & 1u) r[j >> 6] |= 1ull << (j & 63);
    const int CL = MTJ_LIMBS + 1;
    std::vector<uint64_t> c(CL, 0), b(CL, 0), t(CL);
    c[0] = b[0] = 1;
    int L = 0, m = -1;
    for (int step = 0; step < n; ++step) {
        const int off = n - 1 - step, q = off >> 6, sh = off & 63;
        uint64_t acc = 0;
        const int lim = (L >> 6) + 1;
        for (int l = 0; l < lim; ++l) {
            const uint64_t win = sh ? (r[q + l] >> sh) | (r[q + l + 1] << (64 - sh)) : r[q + l];
            acc ^= c[l] & win;
        }
        if (!(__builtin_popcountll(acc) & 1)) continue;
        const int d = step - m, dq = d >> 6, ds = d & 63;      // C ^= B << d
        const bool grow = 2 * L <= step;
        if (grow) t = c;
        for (int l = CL - 1; l >= dq; --l) {
            uint64_t v = b[l - dq] << ds;
            if (ds && l - dq - 1 >= 0) v |= b[l - dq - 1] >> (64 - ds);
            c[l] ^= v;
        }
        if (grow) {
            L = step + 1 - L;
            m = step;
            b = t;
        }
        if (L > MTJ_DEG) return out;     // not this generator
    }
    if (L != MTJ_DEG) return out;
    // reciprocal: phi_i = C_{L-i}
    for (int i = 0; i <= MTJ_DEG; ++i)
        if ((c[(MTJ_DEG - i) >> 6] >> ((MTJ_DEG - i) & 63)) & 1ull) {
            out.p.w[i >> 6] |= 1ull << (i & 63);
            if (i < MTJ_DEG) out.low.push_back(i);
        }
    if (!((out.p.w[MTJ_LIMBS - 1] >> MTJ_TOP) & 1ull) || !(out.p.w[0] & 1ull)) return out;
    // phi must annihilate all 32 bit positions of a sequence it was not derived from
    const int checks = 256;
    const std::vector<uint32_t> y = raw_words(1u, MTJ_DEG + 1 + checks);
    for (int k = 0; k < checks; ++k) {
        uint32_t x = y[k + MTJ_DEG];
        for (int e : out.low) x ^= y[k + e];
        if (x) return out;
    }
    out.ok = true;
    return out;
}

inline const Phi &phi() {
    static const Phi p = derive_phi();     // thread-safe one-time initialisation
    return p;
}

// fold the 624-limb product `v` back below x^19937 (phi is sparse: x^19937 == sum of its lower terms)
inline void reduce(uint64_t *v, const Phi &f, MtPoly &out) {
    auto fold = [&](long base, uint64_t bits) {      // bits = coefficients of x^(19937 + base) .. x^(19937 + base + 63)
        for (int e : f.low) {
            const long s = base + e;
            const int q = (int)(s >> 6), sh = (int)(s & 63);
            v[q] ^= bits << sh;
            if (sh) v[q + 1] ^= bits >> (64 - sh);
        }
    };
    // every term lands strictly below the bit it came from, never above the limb being folded: the loops end
    for (int l = 2 * MTJ_LIMBS - 1; l >= MTJ_LIMBS; --l) {
        uint64_t bits;
        while ((bits = v[l]) != 0) {
            v[l] = 0;
            fold(64l * l - MTJ_DEG, bits);
        }
    }
    const uint64_t high = ~((1ull << MTJ_TOP) - 1ull);
    uint64_t bits;
    while ((bits = v[MTJ_LIMBS - 1] & high) != 0) {
        v[MTJ_LIMBS - 1] ^= bits;
        fold(0, bits >> MTJ_TOP);
    }
    memcpy(out.w, v, sizeof(out.w));
}

inline void mulmod(const MtPoly &a, const MtPoly &b, const Phi &f, MtPoly &out) {
    uint64_t prod[2 * MTJ_LIMBS + 1];
    memset(prod, 0, sizeof(prod));
    uint64_t sh_b[MTJ_LIMBS + 1];
    for (int sh = 0; sh < 64; ++sh) {          // b << sh once, then aligned XORs for every limb of a with bit sh set
        bool any = false;
        for (int l = 0; l < MTJ_LIMBS && !any; ++l) any = (a.w[l] >> sh) & 1ull;
        if (!any) continue;
        sh_b[0] = b.w[0] << sh;
        for (int l = 1; l < MTJ_LIMBS; ++l) sh_b[l] = (b.w[l] << sh) | (sh ? b.w[l - 1] >> (64 - sh) : 0ull);
        sh_b[MTJ_LIMBS] = sh ? b.w[MTJ_LIMBS - 1] >> (64 - sh) : 0ull;
        for (int l = 0; l < MTJ_LIMBS; ++l)
            if ((a.w[l] >> sh) & 1ull)
                for (int k = 0; k <= MTJ_LIMBS; ++k) prod[l + k] ^= sh_b[k];
    }
    reduce(prod, f, out);
}

inline uint64_t spread32(uint64_t x) {   // bit i -> bit 2 i (squaring over GF(2))
    x &= 0xffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return x;
}

inline void sqrmod(const MtPoly &a, const Phi &f, MtPoly &out) {
    uint64_t prod[2 * MTJ_LIMBS + 1];
    for (int l = 0; l < MTJ_LIMBS; ++l) {
        prod[2 * l] = spread32(a.w[l]);
        prod[2 * l + 1] = spread32(a.w[l] >> 32);
    }
    prod[2 * MTJ_LIMBS] = 0;
    reduce(prod, f, out);
}

// x^n mod phi by square-and-multiply (the multiplications are by x: a shift)
inline bool jump_poly(uint64_t n, MtPoly &out) {
    const Phi &f = phi();
    if (!f.ok) return false;
    MtPoly r{};
    r.w[0] = 1;
    for (int bit = 63; bit >= 0; --bit) {
        MtPoly s;
        sqrmod(r, f, s);
        r = s;
        if ((n >> bit) & 1ull) {
            for (int l = MTJ_LIMBS - 1; l > 0; --l) r.w[l] = (r.w[l] << 1) | (r.w[l - 1] >> 63);
            r.w[0] <<= 1;
            if ((r.w[MTJ_LIMBS - 1] >> MTJ_TOP) & 1ull)
                for (int l = 0; l < MTJ_LIMBS; ++l) r.w[l] ^= f.p.w[l];
        }
    }
    out = r;
    return true;
}

}  // namespace mtj
