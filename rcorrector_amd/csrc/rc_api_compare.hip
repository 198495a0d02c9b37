// rc_api_compare.hip -- C ABI, two k-mer tables side by side (include/rcorrector_amd.h: rc_table_compare; kernel in
// rc_compare.hip): the refusals, the device block, and the statistics put together from the two passes' halves.
#include "rc_api_internal.h"
#include "rc_compare.h"

extern "C" {

int rc_table_compare(rc_ctx *a, rc_ctx *b, uint32_t max_bin, uint64_t *cells, rc_table_compare_stats *stats)
{
    if (!a) return RC_ERR_ARG;
    if (!b) {
        rc_set_error(a, "table_compare: the second context is NULL");
        return RC_ERR_ARG;
    }
    if (!cells || max_bin < 1 || max_bin > RC_CMP_MAX_BIN) {
        rc_set_error(a, "table_compare: max_bin must be 1..%d (got %u), cells not NULL", RC_CMP_MAX_BIN, max_bin);
        return RC_ERR_ARG;
    }
    if (!a->d_buckets || !b->d_buckets) {
        rc_set_error(a, "table_compare: no k-mer table loaded in the %s context", !a->d_buckets ? "first" : "second");
        return RC_ERR_STATE;
    }
    if (a->k != b->k) {
        rc_set_error(a, "table_compare: the tables hold k-mers of different length (k = %d and k = %d)", a->k, b->k);
        return RC_ERR_ARG;
    }
    if (a->device != b->device) {
        rc_set_error(a, "table_compare: the contexts sit on different devices (%d and %d): bring one table over with rc_table_replicate first",
                     a->device, b->device);
        return RC_ERR_ARG;
    }
    int rc = rc_drain(b);
    if (rc) {
        rc_lane_error(a, b);
        return rc;
    }
    if ((rc = rc_drain(a))) return rc;
    const size_t nc = rc_cmp_cells(max_bin), words = rc_cmp_out_words(max_bin);
    rc_dev_tmp b_out;
    RC_CHECK_HIP(a, b_out.alloc(words * 8));
    RC_CHECK_HIP(a, hipMemsetAsync(b_out.p, 0, words * 8, a->stream));
    if ((rc = rc_launch_table_compare(a, b, max_bin, b_out.as<unsigned long long>()))) return rc;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t), "64-bit words");
    uint64_t st[2][RC_CMP_STAT_WORDS];
    RC_CHECK_HIP(a, hipMemcpyAsync(cells, b_out.p, nc * 8, hipMemcpyDeviceToHost, a->stream));
    RC_CHECK_HIP(a, hipMemcpyAsync(st, b_out.as<uint64_t>() + nc, sizeof st, hipMemcpyDeviceToHost, a->stream));
    RC_CHECK_HIP(a, hipStreamSynchronize(a->stream));
    if (stats) {
        stats->distinct_a = st[0][RC_CMP_DISTINCT];
        stats->distinct_b = st[1][RC_CMP_DISTINCT];
        stats->shared = st[0][RC_CMP_SHARED];
        stats->mass_a = st[0][RC_CMP_MASS];
        stats->mass_b = st[1][RC_CMP_MASS];
        stats->shared_mass_a = st[0][RC_CMP_SMASS];
        stats->shared_mass_b = st[0][RC_CMP_SMASS_OTHER];
        stats->max_count_a = st[0][RC_CMP_MAX];
        stats->max_count_b = st[1][RC_CMP_MAX];
    }
    return RC_OK;
}

}  // extern "C"
