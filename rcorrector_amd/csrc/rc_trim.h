// rc_trim.h -- read trimming (include/rcorrector_amd.h: rc_read_trim_device): the contract of the three cuts, for the kernel in
// rc_trim.hip and for a host program that runs the lanes one after the other (tests/hostmath/read_trim.cpp).  Integer
// arithmetic only.  The strings are rc_overlap.h's: 2-bit codes and a validity string, 32 bases a 64-bit word.
//
// For a read of L bases (L <= 1023) three independent cuts are taken on the read AS GIVEN, each a position in 0 .. L, L = no cut:
//   cut_q   BWA's / cutadapt's 3' quality rule at threshold q = qual_min: t(j) = q - (Q[j] - qual_base), S(i) = the sum of t(j)
//           over j >= i (S(L) = 0), i0 = the largest i with S(i) < 0 (-1: none); cut_q = the largest i in (i0, L] at which S is
//           maximal.  The stop at i0 is part of the rule: a bad head behind a good middle is not trimmed.  qual_min = 0 or no
//           qualities: L.
//   cut_ad  the mate's adapter, n <= 64 bases of upper-case ACGT: at offset d in 0 .. L - 1 read position i faces adapter base
//           i - d (d <= i < min(L, d + n)); v(d) = the faced positions whose read base is upper-case ACGT, m(d) = those of them
//           that differ; d is accepted if v >= adapter_min and 100 m <= adapter_mm_pct v; cut_ad = the smallest accepted d, else
//           L.  Hamming only.  This is rc_ov_count with the adapter's strings in the place of r (rc_trim_ad_count walks only the
//           three words of the read an adapter of 64 bases can face).
//   cut_pair  d* chosen as the mate-overlap report chooses it (rc_ov_offsets, rc_ov_count, rc_ov_key over mate 1 and the reverse
//           complement of mate 2); F = d* + Lb is the fragment's length: mate 1 keeps min(La, F) bases, mate 2 min(Lb, Lb + d*).
//           No accepted offset, single reads, or the option off: L.
//   keep_len = min(cut_q, cut_ad, cut_pair); a unit (a read, or a pair) is KEPT if every mate has keep_len >= min_len.
//
// The quality scan as the kernel runs it: lane c owns bytes [16 c, 16 c + 16) of the quality string (rc_ov_load16's dwords):
// rc_trim_qual_suffix gives its 16 lane-local suffix sums, a suffix scan over the lanes' totals gives `behind`, the sum of t
// behind the lane's last byte, so S(16 c + k) = suf[k] + behind; one max-reduction of rc_trim_qual_neg gives i0, one of
// rc_trim_qual_best the key of the best position, position L (S = 0) joining as rc_trim_qual_key(0, L).  |t| <= 93 + 255 + 255
// and L <= 1023, so |S| < 2^20: S + 2^21 above the ten bits of the position fits 32 bits.
#pragma once
#include "rc_overlap.h"

#define RC_TRIM_MAX_LEN RC_OV_MAX_LEN
#define RC_TRIM_AD_MAX 64                     // bases of an adapter
#define RC_TRIM_AD_WORDS (RC_TRIM_AD_MAX / 32)  // words of its strings
#define RC_TRIM_QBIAS (1 << 21)

// the adapter's strings; false: n outside 0 .. 64 or a base outside upper-case ACGT
RC_HD bool rc_trim_pack_adapter(const uint8_t *ad, int n, uint64_t *code, uint64_t *val)
{
    for (int w = 0; w < RC_TRIM_AD_WORDS; ++w) code[w] = val[w] = 0;
    if (n < 0 || n > RC_TRIM_AD_MAX) return false;
    for (int i = 0; i < n; ++i) {
        const int c = ad[i] == 'A' ? 0 : ad[i] == 'C' ? 1 : ad[i] == 'G' ? 2 : ad[i] == 'T' ? 3 : -1;
        if (c < 0) return false;
        code[i >> 5] |= (uint64_t)c << (62 - 2 * (i & 31));
        val[i >> 5] |= rc_ov_bit(i);
    }
    return true;
}

// v(d) and m(d) of a read (nwa words that hold a base) against an adapter at offset d >= 0: the adapter faces positions
// d .. d + 63 at most, words d / 32 .. d / 32 + 2; every other word of rc_ov_count's sum is 0
RC_HD void rc_trim_ad_count(const uint64_t *a_code, const uint64_t *a_val, int nwa, const uint64_t *ad_code, const uint64_t *ad_val, int d, int &v, int &m)
{
    v = m = 0;
    const int w0 = d >> 5;
    for (int w = w0; w < nwa && w <= w0 + RC_TRIM_AD_WORDS; ++w) {
        const uint64_t both = a_val[w] & rc_ov_extract(ad_val, RC_TRIM_AD_WORDS, 32 * w - d);
        const uint64_t x = a_code[w] ^ rc_ov_extract(ad_code, RC_TRIM_AD_WORDS, 32 * w - d);
        v += rc_ov_popc(both);
        m += rc_ov_popc((x | (x << 1)) & both);
    }
}

RC_HD bool rc_trim_ad_accepts(int v, int m, int adapter_min, int adapter_mm_pct) { return v >= adapter_min && 100 * m <= adapter_mm_pct * v; }

// suf[k] = the sum of t over bytes k .. 15 of a chunk of which the first `left` bytes (0 .. 16) lie inside the read
RC_HD void rc_trim_qual_suffix(const uint32_t (&w)[4], int left, int q, int qual_base, int (&suf)[16])
{
    int run = 0;
#pragma unroll
    for (int k = 15; k >= 0; --k) {
        const int Q = (int)((w[k >> 2] >> (8 * (k & 3))) & 255u);
        run += k < left ? q - (Q - qual_base) : 0;
        suf[k] = run;
    }
}

// the largest position of the chunk (its first at pos0) with S < 0, else -1
RC_HD int rc_trim_qual_neg(const int (&suf)[16], int behind, int left, int pos0)
{
    int i0 = -1;
#pragma unroll
    for (int k = 0; k < 16; ++k) i0 = k < left && suf[k] + behind < 0 ? pos0 + k : i0;
    return i0;
}

RC_HD uint32_t rc_trim_qual_key(int S, int i) { return ((uint32_t)(S + RC_TRIM_QBIAS) << 10) | (uint32_t)i; }
RC_HD int rc_trim_qual_key_pos(uint32_t key) { return (int)(key & 1023u); }

// the largest key of the chunk's positions behind i0 (0: none): the larger S, then the larger position
RC_HD uint32_t rc_trim_qual_best(const int (&suf)[16], int behind, int left, int pos0, int i0)
{
    uint32_t best = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const uint32_t key = k < left && pos0 + k > i0 ? rc_trim_qual_key(suf[k] + behind, pos0 + k) : 0u;
        best = key > best ? key : best;
    }
    return best;
}

// the pair cut of both mates at the accepted offset ds
RC_HD void rc_trim_pair_cuts(int La, int Lb, int ds, int &cut_a, int &cut_b)
{
    const int F = ds + Lb;
    cut_a = F < La ? F : La;
    cut_b = ds < 0 ? Lb + ds : Lb;
}

RC_HD int rc_trim_keep_len(int cut_q, int cut_ad, int cut_pair)
{
    const int x = cut_q < cut_ad ? cut_q : cut_ad;
    return x < cut_pair ? x : cut_pair;
}
