// rc_depth.h -- the per-read k-mer depth (include/rcorrector_amd.h: rc_read_depth): the rank arithmetic and the selection, for
// the kernel in rc_depth.hip and for a host program (tests/hostmath/depth_select.cpp).
//
// A read's n valid k-windows have the counts c[0] <= ... <= c[n-1]; its four numbers are n, c[(n-1)/4], c[(n-1)/2] and
// c[3(n-1)/4] (lower quantiles; n == 0: four zeros).  Nothing is sorted: the three values are found together by one descent over
// the counts' bits, from the highest bit any count has down to bit 0.  For one rank r the descent keeps a prefix p (the bits of
// the answer above the current one) and r's rank among the counts that share p: at bit b it asks how many of those have bit b
// clear -- c0 -- and either stays among them (r < c0) or sets the bit and moves on among the others (r -= c0).  After bit 0, p is
// the r-th smallest count: every step splits the candidates exactly where the sorted order does, so the result is the sort's,
// ties and all.  The three ranks walk down side by side; while two of them share a prefix they share the question.
// The counts themselves stay wherever the caller keeps them: the selection only asks `count_eq(shift, key)`, the number of
// valid counts v with (v >> shift) == key.  The kernel answers with a ballot and a population count per value slot of its
// lanes, the host program with a loop.
#pragma once
#include "rc_common.h"

#define RC_DEPTH_INVALID 0xFFFFFFFFu  // what stands in a count's place for a window that is not valid (counts are below 2^31)

struct rc_depth_vals {
    int32_t valid, q1, median, q3;
};

RC_HD int rc_depth_fls(uint32_t x)  // index of the highest set bit, x != 0
{
#if defined(__HIP_DEVICE_COMPILE__)
    return 31 - __clz((int)x);
#else
    return 31 - __builtin_clz(x);
#endif
}

// the three ranks of n >= 1 sorted values: (n - 1) / 4 <= (n - 1) / 2 <= 3 (n - 1) / 4, integer division
RC_HD void rc_depth_ranks(uint32_t n, uint32_t (&r)[3])
{
    r[0] = (n - 1u) / 4u;
    r[1] = (n - 1u) / 2u;
    r[2] = 3u * (n - 1u) / 4u;
}

// n: the valid counts; any_or: a value whose highest set bit is that of the largest valid count (their OR, their maximum; 0 when
// all are 0); count_eq(shift, key), 0 <= shift <= 30: the valid counts v with (v >> shift) == key.  RC_DEPTH_INVALID never
// matches: key <= (2^31 - 1) >> shift < 0xFFFFFFFF >> shift.
template <class CountEq>
RC_HD rc_depth_vals rc_depth_select(uint32_t n, uint32_t any_or, CountEq count_eq)
{
    rc_depth_vals d = {(int32_t)n, 0, 0, 0};
    if (n == 0 || any_or == 0) return d;
    uint32_t r[3], p[3] = {0, 0, 0};
    rc_depth_ranks(n, r);
    for (int b = rc_depth_fls(any_or); b >= 0; --b) {
        uint32_t key_prev = 0, c_prev = 0;
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const uint32_t key = p[i] >> b;  // (bit b of p[i] is still clear: the candidates with the bit clear)
            const uint32_t c0 = i > 0 && key == key_prev ? c_prev : (uint32_t)count_eq(b, key);
            key_prev = key;
            c_prev = c0;
            if (r[i] >= c0) {
                r[i] -= c0;
                p[i] |= 1u << b;
            }
        }
    }
    d.q1 = (int32_t)p[0];
    d.median = (int32_t)p[1];
    d.q3 = (int32_t)p[2];
    return d;
}
