// rc_recur.h -- the recurrent-correction census (include/rcorrector_amd.h: rc_recur_census): the arithmetic of its 61-bit site
// keys, for the kernel in rc_recur.hip and for a host program (tests/hostmath/recur_key.cpp).
//
// A CHANGE is a position p of a read at which the byte as it arrived differs from the byte as corrected.  Its WINDOW is the
// 29 bytes after[p - 14 .. p + 14] of the CORRECTED read; the change is CONTEXTED when the window lies inside the read and
// holds upper-case ACGT only, else CLIPPED (counted, no key).  The key:
//   W      the window, 2 bits a base (A C G T = 0 1 2 3), first base in the most significant bits: 58 bits
//   f      0..3: the ORIGINAL byte is upper-case A C G T; 4: anything else (N, lower case, ...)
//   twin   the reverse strand sees the same event as W' = revcomp(W), f' = 3 - f (4 stays 4).  29 is odd: the centre stays
//          the centre, and no base is its own complement, so W != W' always -- the smaller W is canonical, no tie to break
//   key    (W_canon << 3) | f_canon.  The new base is the centre of W_canon, bits 29..28 of W (bits 32..31 of the key)
#pragma once
#include "rc_common.h"

#define RC_RECUR_FLANK 14
#define RC_RECUR_WINDOW (2 * RC_RECUR_FLANK + 1)
#define RC_RECUR_W_MASK ((1ull << (2 * RC_RECUR_WINDOW)) - 1ull)

// 0 1 2 3 = upper-case A C G T, 4 = anything else
RC_HD int rc_recur_from(uint32_t c) { return c == 0x41u ? 0 : (c == 0x43u ? 1 : (c == 0x47u ? 2 : (c == 0x54u ? 3 : 4))); }

RC_HD uint64_t rc_recur_revcomp(uint64_t w) { return rc_revcomp(w, RC_RECUR_WINDOW); }

// the key of window W (58 bits) and from code f (0..4)
RC_HD uint64_t rc_recur_key(uint64_t w, int f)
{
    const uint64_t r = rc_recur_revcomp(w);
    const bool flip = r < w;
    const int fc = flip && f < 4 ? 3 - f : f;
    return ((flip ? r : w) << 3) | (uint64_t)fc;
}

// 32 bytes that start at the window's first, as eight dwords (first byte in the low bits; bytes 29..31 are anything): the
// window packed (rc_pack16m, sixteen bytes per call) into *w; false: one of its 29 bytes is not upper-case ACGT
RC_HD bool rc_recur_window(const uint32_t (&d)[8], uint64_t *w)
{
    const uint32_t d0[4] = {d[0], d[1], d[2], d[3]}, d1[4] = {d[4], d[5], d[6], d[7]};
    uint32_t c0, c1, am, tm, b0, b1;
    rc_pack16m(d0, c0, am, tm, b0);
    rc_pack16m(d1, c1, am, tm, b1);
    (void)am;
    (void)tm;
    *w = ((((uint64_t)c0) << 32) | c1) >> (64 - 2 * RC_RECUR_WINDOW);
    return ((b0 | (b1 << 16)) & ((1u << RC_RECUR_WINDOW) - 1u)) == 0;
}

// position p of a read of L bytes: 0 = no change, 1 = a clipped change, 2 = a contexted one, whose key is in *key -- over
// strings in memory, byte by byte: what a lane of the kernel computes from its aligned pieces
RC_HD int rc_recur_change_at(const uint8_t *before, const uint8_t *after, uint32_t L, uint32_t p, uint64_t *key)
{
    if (before[p] == after[p]) return 0;
    if (p < (uint32_t)RC_RECUR_FLANK || p + (uint32_t)RC_RECUR_FLANK >= L) return 1;
    uint32_t d[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    for (uint32_t i = 0; i < (uint32_t)RC_RECUR_WINDOW; ++i) d[i >> 2] |= (uint32_t)after[p - RC_RECUR_FLANK + i] << (8u * (i & 3u));
    uint64_t w;
    if (!rc_recur_window(d, &w)) return 1;
    *key = rc_recur_key(w, rc_recur_from(before[p]));
    return 2;
}
