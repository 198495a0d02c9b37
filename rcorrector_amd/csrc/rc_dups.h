// rc_dups.h -- the duplicate census (include/rcorrector_amd.h: rc_dup_census): the arithmetic of its 128-bit keys, for the
// kernel in rc_dups.hip and for a host program (tests/hostmath/dup_key.cpp).
//
// A key is two independent 64-bit hashes (lane j = 0, 1: the same construction over two sets of constants).  EQUALITY OF TWO
// UNITS IS DECIDED ON THE KEY ALONE: the strings are never compared again.  Each lane is built so that everything that tells
// two strings apart reaches it through a bijection of 64 bits, and what is folded is folded after such a bijection:
//   chunk    bytes [16 c, 16 c + 16) of the read as two little-endian words (a, b), bytes behind the read's last are 0:
//            h_c = mix(mix(a + (c + 1) * G_j) ^ b ^ S_j) -- a bijection of a for every b and of b for every a, and the chunk's
//            index is in it: two chunks swapped, or one moved, give other terms
//   read     R = fin(sum over c of h_c  +  (L + 1) * N_j), L the length in bytes.  The sum is what the sixteen lanes of a read
//            reduce in any order; the order of the CHUNKS is in the terms.  The length enters on its own: "ACGT" is not "ACGTA"
//            (whose last chunk differs as well), and the empty read has a key
//   pair     U = fin((R1 ^ P_j) * Q_j + mix(R2 + P_j)): not symmetric, so (x, y) is not (y, x), and since each mate's key holds
//            its own length, ("AC", "GT") is not ("ACG", "T").  A single-end unit's key is its read's
// mix / fin are the 64-bit finaliser of MurmurHash3 (Appleby, public domain), a bijection.
#pragma once
#include "rc_common.h"

#define RC_DUP_G0 0x9E3779B97F4A7C15ull
#define RC_DUP_G1 0xD6E8FEB86659FD93ull
#define RC_DUP_S0 0x2545F4914F6CDD1Dull
#define RC_DUP_S1 0x94D049BB133111EBull
#define RC_DUP_N0 0xBF58476D1CE4E5B9ull
#define RC_DUP_N1 0xA0761D6478BD642Full
#define RC_DUP_P0 0xE7037ED1A0B428DBull
#define RC_DUP_P1 0x8EBC6AF09C88C6E3ull
#define RC_DUP_Q0 0x589965CC75374CC3ull  // (odd)
#define RC_DUP_Q1 0x1D8E4E27C47D124Full  // (odd)

RC_HD uint64_t rc_dup_mix(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

// the words of a chunk that holds `rem` bytes of its read (1 <= rem; 16 or more: all of it): the bytes behind them cleared
RC_HD void rc_dup_tail_mask(uint32_t rem, uint64_t &a, uint64_t &b)
{
    // (two masks, no branch over a and b: a compiler that sees "one of the two words, chosen at run time" indexes them in memory)
    const uint64_t ma = rem >= 8u ? ~0ull : (1ull << (8u * rem)) - 1ull;
    const uint64_t mb = rem >= 16u ? ~0ull : (rem <= 8u ? 0ull : (1ull << (8u * (rem - 8u))) - 1ull);
    a &= ma;
    b &= mb;
}

// chunk c's term of lane j
RC_HD uint64_t rc_dup_chunk(uint64_t a, uint64_t b, uint32_t c, int j)
{
    const uint64_t g = j ? RC_DUP_G1 : RC_DUP_G0, s = j ? RC_DUP_S1 : RC_DUP_S0;
    return rc_dup_mix(rc_dup_mix(a + (uint64_t)(c + 1u) * g) ^ b ^ s);
}

// a read's key from the sum of its chunks' terms and its length
RC_HD uint64_t rc_dup_read(uint64_t sum, uint32_t len, int j)
{
    return rc_dup_mix(sum + (uint64_t)(len + 1u) * (j ? RC_DUP_N1 : RC_DUP_N0));
}

// a pair's key from its mates'
RC_HD uint64_t rc_dup_pair(uint64_t r1, uint64_t r2, int j)
{
    const uint64_t p = j ? RC_DUP_P1 : RC_DUP_P0, q = j ? RC_DUP_Q1 : RC_DUP_Q0;
    return rc_dup_mix((r1 ^ p) * q + rc_dup_mix(r2 + p));
}

// the whole of it over a string in memory, byte by byte: what the kernel's sixteen lanes compute between them
RC_HD void rc_dup_read_key(const uint8_t *s, uint32_t len, uint64_t key[2])
{
    uint64_t sum0 = 0, sum1 = 0;
    for (uint32_t c = 0; 16u * c < len; ++c) {
        const uint32_t rem = len - 16u * c, nb = rem < 16u ? rem : 16u;
        uint64_t a = 0, b = 0;
        for (uint32_t i = 0; i < nb; ++i) {
            const uint64_t v = s[16u * c + i];
            if (i < 8u)
                a |= v << (8u * i);
            else
                b |= v << (8u * (i - 8u));
        }
        sum0 += rc_dup_chunk(a, b, c, 0);
        sum1 += rc_dup_chunk(a, b, c, 1);
    }
    key[0] = rc_dup_read(sum0, len, 0);
    key[1] = rc_dup_read(sum1, len, 1);
}

RC_HD void rc_dup_pair_key(const uint8_t *s1, uint32_t len1, const uint8_t *s2, uint32_t len2, uint64_t key[2])
{
    uint64_t k1[2], k2[2];
    rc_dup_read_key(s1, len1, k1);
    rc_dup_read_key(s2, len2, k2);
    key[0] = rc_dup_pair(k1[0], k2[0], 0);
    key[1] = rc_dup_pair(k1[1], k2[1], 1);
}
