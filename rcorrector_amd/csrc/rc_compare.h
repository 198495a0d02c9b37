// rc_compare.h -- what the comparison kernel (rc_compare.hip) and its entry point (rc_api_compare.hip) agree on: the
// limits, the layout of the device block, and the fold / cell arithmetic (constexpr: host and device).
#pragma once
#include <stddef.h>
#include <stdint.h>

#define RC_CMP_MAX_BIN 1023  // (max_bin + 1)^2 64-bit cells: at most 8 MiB on the device
#define RC_CMP_CORNER 32     // cells (i, j) with i, j < RC_CMP_CORNER are privatised per workgroup in LDS (4 KiB)

// the device block behind the cells: two passes' statistics, RC_CMP_STAT_WORDS 64-bit words each -- of the SCANNED table's
// live entries: distinct, mass, max; pass 0 also: k-mers the probed table holds too, their mass here and over there
enum { RC_CMP_DISTINCT = 0, RC_CMP_MASS, RC_CMP_MAX, RC_CMP_SHARED, RC_CMP_SMASS, RC_CMP_SMASS_OTHER, RC_CMP_STAT_WORDS };

constexpr size_t rc_cmp_cells(uint32_t max_bin) { return ((size_t)max_bin + 1) * ((size_t)max_bin + 1); }
constexpr size_t rc_cmp_out_words(uint32_t max_bin) { return rc_cmp_cells(max_bin) + 2 * RC_CMP_STAT_WORDS; }
// a count as the matrix sees it: exact below max_bin, the last bin holds "at least max_bin"
constexpr uint32_t rc_cmp_fold(uint32_t count, uint32_t max_bin) { return count < max_bin ? count : max_bin; }

struct rc_ctx;
// both passes on a's stream (a's device current, both tables on it): d_out = rc_cmp_out_words(max_bin) words, zeroed by the caller
int rc_launch_table_compare(rc_ctx *a, const rc_ctx *b, uint32_t max_bin, unsigned long long *d_out);
