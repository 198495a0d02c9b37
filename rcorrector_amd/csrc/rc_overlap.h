// rc_overlap.h -- the mate-overlap report (include/rcorrector_amd.h: rc_mate_overlap): the per-pair arithmetic -- pack, scan the
// offsets, choose d*, classify the faced positions -- for the kernel in rc_overlap.hip and for a host program that runs the
// lanes one after the other (tests/hostmath/mate_overlap.cpp).
//
// A mate is a STRING of nw 64-bit words, 32 bases a word, base i in word i / 32 at the field of bits 63 - 2 (i % 32) (high) and
// 62 - 2 (i % 32) (low) -- rc_pack16m's order, first base in the top bits.  Two strings a mate: `code`, the 2-bit codes, and
// `val`, whose field's HIGH bit says "this base is one of upper-case ACGT" (its low bit is always 0).  val is 0 for every
// position at or behind the mate's end, so a position outside a mate is never valid and no loop below needs the lengths.
// Mate 2 is held as r, its reverse complement: r[j] = comp(b[Lb - 1 - j]).
//
// At offset d, a[i] faces r[i - d].  Word w of "r moved by d" is the 32 bases of r from 32 w - d on (rc_ov_extract: two
// words funnel-shifted; words outside the string are 0).  Then for word w of a:
//   both = val_a[w] & val_r'[w]                     faced positions where both bases are valid
//   x = code_a[w] ^ code_r'[w];  differ = (x | x << 1) & both     ... and differ
// and v(d), m(d) are the population counts over the words.
#pragma once
#include "rc_common.h"

#define RC_OV_FIELD_HI 0xAAAAAAAAAAAAAAAAull
#define RC_OV_MAX_LEN 1023   // bases of a mate that are looked at (the reference's reads hold no more, utils.h:7)
#define RC_OV_FRAG 2048      // rc_mate_overlap::frag
#define RC_OV_POS 1024       // positions of the per-position arrays (rcorrector_amd.h: RC_OVERLAP_MAX_LEN)

RC_HD int rc_ov_popc(uint64_t x)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __popcll(x);
#else
    return __builtin_popcountll(x);
#endif
}

RC_HD uint32_t rc_ov_spread16(uint32_t x)  // bit j of x (j < 16) -> bit 2 j
{
    x &= 0xFFFFu;
    x = (x | (x << 8)) & 0x00FF00FFu;
    x = (x | (x << 4)) & 0x0F0F0F0Fu;
    x = (x | (x << 2)) & 0x33333333u;
    x = (x | (x << 1)) & 0x55555555u;
    return x;
}

// 16 bytes (four dwords, first byte in the low bits; bytes behind a read's end as 0) -> half a word of the two strings
RC_HD void rc_ov_pack16(const uint32_t (&w)[4], uint32_t &code, uint32_t &val)
{
    uint32_t am, tm, bad;
    rc_pack16m(w, code, am, tm, bad);
    val = rc_brev32(rc_ov_spread16(~bad));  // byte j valid -> bit 31 - 2 j, the high bit of its field
}

// the 32 bases of a string from base s on (s may be negative or reach past the string: what is not there is 0)
RC_HD uint64_t rc_ov_extract(const uint64_t *str, int nw, int s)
{
    const int q = s >> 5, t = s & 31;  // (arithmetic shift: floor)
    const uint64_t lo = (unsigned)q < (unsigned)nw ? str[q] : 0ull;
    if (t == 0) return lo;
    const uint64_t hi = (unsigned)(q + 1) < (unsigned)nw ? str[q + 1] : 0ull;
    return (lo << (2 * t)) | (hi >> (64 - 2 * t));
}

// a word with its 32 fields in reverse order (field f -> field 31 - f, each field's two bits kept in place)
RC_HD uint64_t rc_ov_rev_fields(uint64_t x)
{
    x = rc_brev64(x);
    return ((x & 0x5555555555555555ull) << 1) | ((x >> 1) & 0x5555555555555555ull);
}

// Word w of r's strings from b's (nw words each, Lb bases): b's padded string reversed field by field is r behind
// 32 nw - Lb fields of padding, so r's word w starts 32 w + 32 nw - Lb fields into it.  comp: the codes are complemented
// (A <-> T, C <-> G: 3 - c), the validity string is not.
RC_HD uint64_t rc_ov_rc_word(const uint64_t *b_str, int nw, int Lb, int w, bool comp)
{
    const int s = 32 * w + 32 * nw - Lb;
    const int q = s >> 5, t = s & 31;
    // reversed string word q = rev_fields(b_str[nw - 1 - q])
    const uint64_t lo = (unsigned)q < (unsigned)nw ? rc_ov_rev_fields(b_str[nw - 1 - q]) : 0ull;
    uint64_t x = lo;
    if (t) {
        const uint64_t hi = (unsigned)(q + 1) < (unsigned)nw ? rc_ov_rev_fields(b_str[nw - 2 - q]) : 0ull;
        x = (lo << (2 * t)) | (hi >> (64 - 2 * t));
    }
    return comp ? ~x : x;
}

// the offsets worth a look: an overlap of fewer than min_overlap positions cannot reach v >= min_overlap
RC_HD void rc_ov_offsets(int La, int Lb, int min_overlap, int &d_lo, int &d_hi)  // d_lo > d_hi: none
{
    d_lo = min_overlap - Lb > -(Lb - 1) ? min_overlap - Lb : -(Lb - 1);
    d_hi = La - min_overlap < La - 1 ? La - min_overlap : La - 1;
    if (La < min_overlap || Lb < min_overlap) {
        d_lo = 0;
        d_hi = -1;
    }
}

// v(d) and m(d)
RC_HD void rc_ov_count(const uint64_t *a_code, const uint64_t *a_val, int nwa, const uint64_t *r_code, const uint64_t *r_val, int nwr, int d, int &v,
                       int &m)
{
    v = m = 0;
    for (int w = 0; w < nwa; ++w) {
        const uint64_t both = a_val[w] & rc_ov_extract(r_val, nwr, 32 * w - d);
        const uint64_t x = a_code[w] ^ rc_ov_extract(r_code, nwr, 32 * w - d);
        v += rc_ov_popc(both);
        m += rc_ov_popc((x | (x << 1)) & both);
    }
}

// The key of an offset: 0 if it is not accepted, else larger for the better offset -- the larger v, then the smaller m, then
// the smaller d.  v, m <= RC_OV_MAX_LEN (10 bits each), d + RC_OV_MAX_LEN in 1 .. 2 RC_OV_MAX_LEN - 1 (11 bits).
RC_HD uint32_t rc_ov_key(int v, int m, int d, int min_overlap, int max_mismatch_pct)
{
    if (v < min_overlap || 100 * m > max_mismatch_pct * v) return 0u;
    return ((uint32_t)v << 21) | ((uint32_t)(RC_OV_MAX_LEN - m) << 11) | (uint32_t)(2047 - (d + RC_OV_MAX_LEN));
}
RC_HD int rc_ov_key_d(uint32_t key) { return 2047 - (int)(key & 2047u) - RC_OV_MAX_LEN; }

// word w of a at offset d, in one version: the positions where both bases are valid, and those where they differ too
struct rc_ov_faced {
    uint64_t both, differ;
};
RC_HD rc_ov_faced rc_ov_face(const uint64_t *a_code, const uint64_t *a_val, const uint64_t *r_code, const uint64_t *r_val, int nwr, int d, int w)
{
    rc_ov_faced f;
    f.both = a_val[w] & rc_ov_extract(r_val, nwr, 32 * w - d);
    const uint64_t x = a_code[w] ^ rc_ov_extract(r_code, nwr, 32 * w - d);
    f.differ = (x | (x << 1)) & f.both;
    return f;
}
// the bit of position i (of a) in such a word: word i / 32, this bit
RC_HD uint64_t rc_ov_bit(int i) { return 1ull << (63 - 2 * (i & 31)); }
