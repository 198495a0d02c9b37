// rc_norm.h -- normalisation by k-mer depth (include/rcorrector_amd.h: rc_norm_select_device): the selection's contract, for the
// kernel in rc_norm.hip and for a host program (tests/hostmath/norm_select.cpp).  Integer arithmetic only.
//
// The scheme is after Trinity's in-silico normalisation with --pairs_together: the mates' median k-mer coverages averaged, the
// unit kept with probability max_cov / median.  Neither its random stream nor byte parity with it is claimed.  Its
// coefficient-of-variation filter has no counterpart here.
//   unit     a read (mode 0), read u with read n_units + u (mode 1), reads 2u and 2u + 1 (mode 2): the duplicate census's modes
//   depth D  of the rc_read_depth of the unit's mates, those with valid > 0 only: one such mate -- its median; two --
//            (m1 + m2 + 1) >> 1, unsigned (medians are below 2^31: no overflow); none -- the unit is NOVALID
//   draw r   the upper 32 bits of the splitmix64 finaliser of seed + (index + 1) * 0x9E3779B97F4A7C15, index the unit's number
//            in the WHOLE input, 64 bits, not its number in a batch: the decision depends on (seed, index, D) alone, so a run is
//            reproducible and the same however the input is cut into batches
//   outcome  NOVALID without a valid mate; else LOW if D < min_cov; else KEPT if D <= target or r * D < target * 2^32 (64-bit
//            products: target < 2^31, D < 2^31); else OVER.  A unit is kept with probability min(1, target / D) to within 2^-32.
//   bin      min(D, max_bin) of the unit-depth histograms: `before` over the units that are not NOVALID, `after` over the KEPT
#pragma once
#include "rc_common.h"

// (the values of include/rcorrector_amd.h, token for token)
#define RC_NORM_OVER 0
#define RC_NORM_KEPT 1
#define RC_NORM_LOW 2
#define RC_NORM_NOVALID 3

// valid / median of the unit's mates (a single read: valid2 = 0); false: no mate with a valid window, *depth is 0 then
RC_HD bool rc_norm_unit_depth(int32_t valid1, int32_t median1, int32_t valid2, int32_t median2, uint32_t *depth)
{
    const bool a = valid1 > 0, b = valid2 > 0;
    const uint32_t m1 = (uint32_t)median1, m2 = (uint32_t)median2;
    *depth = a && b ? (m1 + m2 + 1u) >> 1 : a ? m1 : b ? m2 : 0u;
    return a || b;
}

RC_HD uint32_t rc_norm_draw(uint64_t seed, uint64_t index)
{
    uint64_t z = seed + (index + 1u) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(z >> 32);
}

RC_HD uint32_t rc_norm_outcome(bool has_valid, uint32_t depth, uint32_t draw, uint32_t target, uint32_t min_cov)
{
    if (!has_valid) return RC_NORM_NOVALID;
    if (depth < min_cov) return RC_NORM_LOW;
    if (depth <= target || (uint64_t)draw * depth < (uint64_t)target << 32) return RC_NORM_KEPT;
    return RC_NORM_OVER;
}

RC_HD uint32_t rc_norm_bin(uint32_t depth, uint32_t max_bin) { return depth < max_bin ? depth : max_bin; }
