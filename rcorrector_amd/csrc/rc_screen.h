// rc_screen.h -- the per-read hit profile against a second k-mer set (include/rcorrector_amd.h: rc_read_screen): the arithmetic
// on a read's hit mask, for the kernel in rc_screen.hip and for a host program (tests/hostmath/screen_mask.cpp).
//
// A read's nwin k-windows are one bit each, window i at bit i & 63 of 64-bit word i >> 6 (at most RC_MAX_READ_LENGTH / 64
// words): set where the window is a HIT.  Nothing is kept per base or per window; the words are walked once, in order, one
// step per RUN of equal bits (a count-trailing-zeros on the word or its complement), and four numbers are carried along:
//   hits     the set bits
//   longest  the longest run of set bits; `run`, the length of the run of set bits that ends at the last bit seen, carries a
//            run across a word boundary
//   covered  the bases inside at least one hit window, the union of the intervals [i, i + k) over the hits i.  Take the hits in
//            ascending order and give each hit i the bases [i, min(i + k, j)), j the next hit (the last hit: [i, i + k)).  These
//            pieces are disjoint -- each ends where the next begins, or before -- and their union is the intervals' union: a base
//            of [i, i + k) at or past j lies in [j, j + k) as well, or in a later hit's interval, since j - i < k there and the
//            same argument applies to j.  So covered = the sum over the hits of min(k, next_hit(i) - i), the last hit counting k.
//            Run by run: a hit followed by a hit gives 1, a hit followed by z >= 1 misses and then a hit gives 1 + min(k - 1, z),
//            the last hit gives 1 + (k - 1).  `gap`, the misses since the last hit, carries a gap across a word boundary.
// An invalid window is no hit: it ends a run like any miss.  The kernel's words are its wavefronts' ballots, the host program's
// an array.
#pragma once
#include "rc_common.h"

struct rc_screen_vals {
    int32_t valid, hits, covered, longest;
};

struct rc_screen_acc {
    uint32_t hits = 0, covered = 0, longest = 0;
    uint32_t run = 0;  // set bits at the end of what has been seen
    uint32_t gap = 0;  // clear bits since the last set bit (meaningful once hits > 0)
};

RC_HD uint32_t rc_screen_ctz(uint64_t x)  // index of the lowest set bit, x != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return (uint32_t)(__ffsll((unsigned long long)x) - 1);
#else
    return (uint32_t)__builtin_ctzll(x);
#endif
}

// the next word of the mask: bits [0, nbits) of `hit` are windows, 1 <= nbits <= 64, the bits at and above nbits are clear
RC_HD void rc_screen_add_word(rc_screen_acc &a, uint64_t hit, uint32_t nbits, int k)
{
    for (uint32_t pos = 0; pos < nbits;) {
        const uint64_t x = hit >> pos;
        if (x & 1u) {
            const uint64_t z = ~x;  // (the bits shifted in are clear: z has a set bit at or below 64 - pos, except for pos == 0 and a full word)
            const uint32_t ones = z ? rc_screen_ctz(z) : 64u;
            if (a.run == 0 && a.hits) a.covered += a.gap < (uint32_t)k - 1u ? a.gap : (uint32_t)k - 1u;  // the last hit in front of the gap
            a.gap = 0;
            a.run += ones;
            a.hits += ones;
            a.covered += ones;
            a.longest = a.run > a.longest ? a.run : a.longest;
            pos += ones;
        } else {
            const uint32_t zeros = x ? rc_screen_ctz(x) : nbits - pos;
            a.run = 0;
            a.gap += zeros;
            pos += zeros;
        }
    }
}

// after the last word; valid: the read's valid windows, counted by the caller
RC_HD rc_screen_vals rc_screen_finish(const rc_screen_acc &a, uint32_t valid, int k)
{
    rc_screen_vals v = {(int32_t)valid, (int32_t)a.hits, (int32_t)(a.covered + (a.hits ? (uint32_t)k - 1u : 0u)), (int32_t)a.longest};
    return v;
}

// a whole mask at once: hit[(nwin + 63) / 64] as above, the bits at and above nwin clear
RC_HD rc_screen_vals rc_screen_mask(const uint64_t *hit, uint32_t nwin, uint32_t valid, int k)
{
    rc_screen_acc a;
    for (uint32_t w = 0; 64u * w < nwin; ++w) rc_screen_add_word(a, hit[w], nwin - 64u * w < 64u ? nwin - 64u * w : 64u, k);
    return rc_screen_finish(a, valid, k);
}
