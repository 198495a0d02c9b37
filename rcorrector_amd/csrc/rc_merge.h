// rc_merge.h -- merging overlapping mates (include/rcorrector_amd.h: rc_read_merge_device): the contract, for the kernels in
// rc_merge.hip and for a host program that runs the lanes one after the other (tests/hostmath/read_merge.cpp).  Integer
// arithmetic only.
//
// A pair is a (mate 1, La bases, quality bytes qa) and b (mate 2, Lb, qb); r is the reverse complement of b, r[j] =
// comp(b[Lb - 1 - j]) with quality qr[j] = qb[Lb - 1 - j]; at offset d, a[i] faces r[i - d] (rc_overlap.h).
//   d*      chosen exactly as the mate-overlap report and the pair cut of rc_trim.h choose it: rc_ov_offsets, rc_ov_count and
//           rc_ov_key with min_overlap and max_mismatch_pct over the bases as given, the largest key.  No accepted offset: the
//           pair is UNMERGED, merged_len = 0 and d = v = m = 0 in its row.
//   F       = d* + Lb, the merged length (rc_trim.h's fragment length).  Position p in 0 .. F - 1 is covered by a when p < La
//           and by r, at r[p - d*], when p >= d*; every p is covered by one of them at least.  What lies outside is read-through
//           and is dropped: r[0 .. -d* - 1] for d* < 0, a[F ..] for F < La.
//   per position (rc_merge_at), a base VALID when it is upper-case ACGT, the phred value p(Q) = max(0, Q - qual_base):
//           covered by one mate       that mate's base byte (mate 2's through rc_merge_comp) and quality byte, verbatim
//           both valid and equal      that base, quality qual_base + min(pa + pb, qual_cap)
//           both valid and different  the mate with the larger phred value wins, a tie goes to mate 1; quality
//                                     qual_base + min(max(|pa - pb|, 2), qual_cap)
//           exactly one valid         that mate's base byte and quality byte, verbatim
//           neither valid             mate 1's two bytes, verbatim
//           without qualities         a disagreement keeps mate 1's base (it counts as a tie); no quality is made
// F <= La + Lb - min_overlap <= 2045.  Of a read longer than 1023 bases the trimming and overlap kernels look at the first 1023
// only; the kernels that stage reads in the probe tile (depth, screen, weak profile) take it as no read: four zeros.
//
// The write as the kernel does it (rc_merge_granule): the unit's F + 1 output bytes -- the merged read and its NUL -- lie at
// [beg, beg + F + 1) of the output arena; a lane makes one ALIGNED 16-byte granule of the arena: byte k of the granule whose
// first byte is merged position p0 (negative in the unit's first granule when beg is not a multiple of 16) is position p0 + k,
// ours if 0 <= p0 + k <= F.  A granule that is ours in all 16 bytes goes out as one store, any other byte by byte.
#pragma once
#include "rc_overlap.h"

#define RC_MERGE_MAX_LEN RC_OV_MAX_LEN                // bases of a mate
#define RC_MERGE_LEN_BINS 2048                        // rc_merge_tally::len_hist
#define RC_MERGE_MAX_OUT (2 * RC_MERGE_MAX_LEN - 1)   // bases of a merged read

struct rc_merge_rule {
    int min_overlap, max_mismatch_pct, qual_base, qual_cap;
};

RC_HD bool rc_merge_rule_ok(const rc_merge_rule &R)
{
    return R.min_overlap >= 1 && R.min_overlap <= RC_MERGE_MAX_LEN && R.max_mismatch_pct >= 0 && R.max_mismatch_pct <= 50 && R.qual_base >= 0 &&
           R.qual_cap >= 2 && R.qual_cap <= 93 && R.qual_base + R.qual_cap <= 126;
}

RC_HD bool rc_merge_valid(uint8_t c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; }

// ACGT <-> TGCA, acgt <-> tgca, every other byte as it is
RC_HD uint8_t rc_merge_comp(uint8_t c)
{
    switch (c) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'a': return 't';
    case 'c': return 'g';
    case 'g': return 'c';
    case 't': return 'a';
    default: return c;
    }
}

// a unit's mates as bytes (LDS in the kernel) and what the plan chose for it; qa == qb == null: no qualities
struct rc_merge_unit {
    const uint8_t *a, *qa, *b, *qb;
    int La, Lb, d, F;
};

enum { RC_MERGE_TOOK_NONE = 0, RC_MERGE_TOOK_1 = 1, RC_MERGE_TOOK_2 = 2, RC_MERGE_TOOK_TIE = 3 };

// position p (0 <= p < F) of the merged read; took: which mate a disagreement went to (RC_MERGE_TOOK_NONE: it is none)
RC_HD void rc_merge_at(const rc_merge_rule &R, const rc_merge_unit &U, int p, uint8_t &base, uint8_t &qual, int &took)
{
    took = RC_MERGE_TOOK_NONE;
    const bool in_a = p < U.La, in_r = p >= U.d;
    const int jb = U.Lb - 1 - (p - U.d);  // the position of b that faces p
    const bool has_q = U.qa != nullptr;
    const uint8_t ca = in_a ? U.a[p] : 0, cr = in_r ? rc_merge_comp(U.b[jb]) : 0;
    const uint8_t ka = in_a && has_q ? U.qa[p] : 0, kr = in_r && has_q ? U.qb[jb] : 0;
    if (!in_r || !in_a) {
        base = in_a ? ca : cr;
        qual = in_a ? ka : kr;
        return;
    }
    const bool va = rc_merge_valid(ca), vr = rc_merge_valid(cr);
    if (!va || !vr) {  // exactly one valid: that mate's; neither: mate 1's
        const bool second = vr && !va;
        base = second ? cr : ca;
        qual = second ? kr : ka;
        return;
    }
    const int pa = (int)ka - R.qual_base < 0 ? 0 : (int)ka - R.qual_base, pr = (int)kr - R.qual_base < 0 ? 0 : (int)kr - R.qual_base;
    if (ca == cr) {
        const int s = pa + pr;
        base = ca;
        qual = (uint8_t)(R.qual_base + (s < R.qual_cap ? s : R.qual_cap));
        return;
    }
    if (!has_q) {
        base = ca;
        qual = 0;
        took = RC_MERGE_TOOK_TIE;
        return;
    }
    int diff = pa - pr;
    took = diff > 0 ? RC_MERGE_TOOK_1 : diff < 0 ? RC_MERGE_TOOK_2 : RC_MERGE_TOOK_TIE;
    base = diff >= 0 ? ca : cr;
    diff = diff < 0 ? -diff : diff;
    diff = diff < 2 ? 2 : diff;
    qual = (uint8_t)(R.qual_base + (diff < R.qual_cap ? diff : R.qual_cap));
}

// The 16 bytes of the output granule whose first byte is merged position p0, as four dwords (first byte in the low bits), of
// the sequence and of the qualities; position F is the NUL.  Returns the mask of the bytes that are the unit's (bit k: position
// p0 + k lies in 0 .. F), the others are 0 in the dwords and must not be stored.  tk[0 .. 2] += the disagreements that went to
// mate 1, to mate 2, and the ties.
RC_HD uint32_t rc_merge_granule(const rc_merge_rule &R, const rc_merge_unit &U, int p0, uint32_t (&ws)[4], uint32_t (&wq)[4], uint32_t (&tk)[3])
{
    uint32_t mask = 0;
    ws[0] = ws[1] = ws[2] = ws[3] = 0;
    wq[0] = wq[1] = wq[2] = wq[3] = 0;
    for (int k = 0; k < 16; ++k) {
        const int p = p0 + k;
        if (p < 0 || p > U.F) continue;
        mask |= 1u << k;
        if (p == U.F) continue;  // the NUL
        uint8_t base, qual;
        int took;
        rc_merge_at(R, U, p, base, qual, took);
        ws[k >> 2] |= (uint32_t)base << (8 * (k & 3));
        wq[k >> 2] |= (uint32_t)qual << (8 * (k & 3));
        tk[0] += took == RC_MERGE_TOOK_1 ? 1u : 0u;
        tk[1] += took == RC_MERGE_TOOK_2 ? 1u : 0u;
        tk[2] += took == RC_MERGE_TOOK_TIE ? 1u : 0u;
    }
    return mask;
}

// the row of a unit from the best key of its offset scan (0: no accepted offset): merged_len, d, v, m
RC_HD void rc_merge_row(uint32_t best, int Lb, int &merged_len, int &d, int &v, int &m)
{
    merged_len = d = v = m = 0;
    if (best == 0) return;
    d = rc_ov_key_d(best);
    v = (int)(best >> 21);
    m = RC_OV_MAX_LEN - (int)((best >> 11) & 1023u);
    merged_len = d + Lb;
}

// merged with a part of a mate dropped
RC_HD bool rc_merge_readthrough(int La, int d, int F) { return d < 0 || F < La; }
