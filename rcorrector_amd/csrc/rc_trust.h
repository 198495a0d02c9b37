// rc_trust.h -- the k-mer trust profile by read position (include/rcorrector_amd.h: rc_trust_profile): the word-level
// arithmetic of its accumulate, for the kernel in rc_trust.hip and for a host program (tests/hostmath/trust_words.cpp).
//
// The planes are rc_weak.h's: one bit per arena byte, bit (p & 63) of word p >> 6 = the k-window that starts at byte p is
// SOLID / WEAK.  A read whose first base is bit `bit0` of a plane has the windows 0 .. nwin - 1, its WINDOW STRING.  The
// accumulate takes that string 64 windows a word, one window per lane, twice:
//   from the 5' end   word j = windows [64 j, 64 j + 64): bit l is the window at p5 = 64 j + l          (rc_weak_word)
//   from the 3' end   word j = windows [nwin - 64 (j + 1), nwin - 64 j), reversed: bit l is the window at p3 = 64 j + l,
//                     p3 = 0 the read's last window                                                     (rc_trust_word3)
// Either word has no bit set outside the read's windows, so a lane adds its bit without looking at nwin again.
#pragma once
#include "rc_weak.h"

#define RC_TRUST_LEN 1024  // positions a profile holds (rcorrector_amd.h: RC_TRUST_MAX_LEN)

RC_HD uint64_t rc_trust_rev(uint64_t x)  // bit l of the result = bit 63 - l of x
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __brevll(x);
#else
    x = ((x >> 1) & 0x5555555555555555ull) | ((x & 0x5555555555555555ull) << 1);
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    x = ((x >> 8) & 0x00FF00FF00FF00FFull) | ((x & 0x00FF00FF00FF00FFull) << 8);
    x = ((x >> 16) & 0x0000FFFF0000FFFFull) | ((x & 0x0000FFFF0000FFFFull) << 16);
    return (x >> 32) | (x << 32);
#endif
}

// the windows a read of L bases has at k, cut to what a profile holds
RC_HD uint32_t rc_trust_nwin(int32_t L, int k)
{
    if (L < k) return 0;
    const uint32_t n = (uint32_t)(L - k + 1);
    return n < (uint32_t)RC_TRUST_LEN ? n : (uint32_t)RC_TRUST_LEN;
}

// word j of a read's windows taken right-aligned (nwin > 64 j): the 64 windows that end at window nwin - 1 - 64 j, reversed.
// Where fewer than 64 are left the string starts inside the word -- its start, nwin - 64 (j + 1), is negative: what lies in
// front of window 0 in the plane belongs to another read, so the word is cut to the `left` windows there are (the mask)
// and moved up, which leaves the positions in front of window 0 clear.  Reads the plane words rc_weak_word reads for those
// windows and no other.
RC_HD uint64_t rc_trust_word3(const uint64_t *plane, uint64_t bit0, uint32_t j, uint32_t nwin)
{
    const uint32_t left = nwin - 64u * j;
    if (left >= 64u) return rc_trust_rev(rc_weak_word(plane, bit0 + (left - 64u), 0, 64u));
    return rc_trust_rev(rc_weak_word(plane, bit0, 0, left) << (64u - left));
}

// bit l of the windows word: lanes 64 j + l < nwin hold a window
RC_HD uint64_t rc_trust_have(uint32_t j, uint32_t nwin)
{
    const uint32_t left = nwin - 64u * j;
    return left < 64u ? (1ull << left) - 1ull : ~0ull;
}
