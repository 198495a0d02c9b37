// rc_weak.h -- the per-read weak-k-mer profile (include/rcorrector_amd.h: rc_read_weak): the word-level arithmetic of its
// reduce, for the kernel in rc_weak.hip and for a host program (tests/hostmath/weak_reduce.cpp).
//
// Two bit planes over an arena, one bit per byte, bit (p & 63) of word p >> 6 = the k-window that starts at byte p is SOLID
// (all upper-case ACGT, inside one read, count >= min_count) / WEAK (the same with a smaller count).  A read of L bases whose
// first base is bit `bit0` of the planes has the windows 0 .. L - k; its four numbers are
//   weak        the weak windows
//   bad_prefix  start of the first solid window
//   bad_suffix  L - (start of the last solid window + k)
//   uncovered   L - the bases that lie in a solid window
// with bad_prefix = bad_suffix = uncovered = L for a read without a solid window.  Bits outside a read's windows are ignored.
#pragma once
#include "rc_common.h"

struct rc_weak_vals {
    int32_t weak, bad_prefix, bad_suffix, uncovered;
};

RC_HD int rc_weak_popc(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

RC_HD int rc_weak_ffs(uint64_t x)  // index of the lowest set bit, x != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffsll((unsigned long long)x) - 1;
#else
    return __builtin_ctzll(x);
#endif
}

RC_HD int rc_weak_fls(uint64_t x)  // index of the highest set bit, x != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return 63 - __clzll((long long)x);
#else
    return 63 - __builtin_clzll(x);
#endif
}

// word j of a read's windows: bits [bit0 + 64 j, bit0 + 64 j + 64) of the plane, cut to the nwin windows the read has
// (nwin > 64 j).  Reads plane words (bit0 + 64 j) >> 6 and, only where the 64 bits straddle two, the next one.
RC_HD uint64_t rc_weak_word(const uint64_t *plane, uint64_t bit0, uint32_t j, uint32_t nwin)
{
    const uint64_t b = bit0 + 64ull * j;
    const uint32_t s = (uint32_t)(b & 63u), left = nwin - 64u * j;
    uint64_t v = plane[b >> 6] >> s;
    if (s && left > 64u - s) v |= plane[(b >> 6) + 1] << (64u - s);
    return left < 64u ? v & ((1ull << left) - 1ull) : v;
}

// (cur << d) with the top d bits of prev shifted in, 0 <= d < 64
RC_HD uint64_t rc_weak_shl(uint64_t cur, uint64_t prev, int d)
{
    return d ? (cur << d) | (prev >> (64 - d)) : cur;
}

// bases covered by the solid windows of `cur` and of the word before it, `prev`: bit p of the result = some window
// starting at p - k + 1 .. p is solid (1 <= k <= 64).  Shift-and-OR doubling: after the step of width w a set bit has grown
// to min(2 w, k) bits; prev takes the same steps, its low bits wrong where the word before it would have carried in --
// they never travel the 64 - k bits to its top, which is all that reaches cur.
RC_HD uint64_t rc_weak_dilate(uint64_t cur, uint64_t prev, int k)
{
    int w = 1;
    while (2 * w <= k) {
        cur |= rc_weak_shl(cur, prev, w);
        prev |= prev << w;
        w *= 2;
    }
    if (k > w) cur |= rc_weak_shl(cur, prev, k - w);
    return cur;
}

// the four numbers of one read: L bases from bit `bit0` of the two planes
RC_HD rc_weak_vals rc_weak_reduce(const uint64_t *solid, const uint64_t *weak, uint64_t bit0, int32_t L, int k)
{
    rc_weak_vals r;
    r.weak = 0;
    if (L < 0) L = 0;
    r.bad_prefix = r.bad_suffix = r.uncovered = L;
    if (L < k) return r;
    const uint32_t nwin = (uint32_t)(L - k + 1);
    int first = -1, last = -1, covered = 0;
    uint64_t prev = 0;
    // (the last windows' bases reach k - 1 bits past the last window: one more word where they cross into it)
    const uint32_t nw = (nwin + 63u) / 64u, nw_cov = ((uint32_t)L + 63u) / 64u;
    for (uint32_t j = 0; j < nw_cov; ++j) {
        uint64_t s = 0;
        if (j < nw) {
            s = rc_weak_word(solid, bit0, j, nwin);
            r.weak += rc_weak_popc(rc_weak_word(weak, bit0, j, nwin));
            if (s) {
                if (first < 0) first = (int)(64u * j) + rc_weak_ffs(s);
                last = (int)(64u * j) + rc_weak_fls(s);
            }
        }
        covered += rc_weak_popc(rc_weak_dilate(s, prev, k));
        prev = s;
    }
    if (first >= 0) {
        r.bad_prefix = first;
        r.bad_suffix = L - (last + k);
        r.uncovered = L - covered;
    }
    return r;
}
