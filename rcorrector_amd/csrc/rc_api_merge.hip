// rc_api_merge.hip -- C ABI, read merging (include/rcorrector_amd.h: rc_read_merge_device; the contract in rc_merge.h, the kernels
// in rc_merge.hip): the device entry point.  The merge reads bases and qualities, not k-mers: it needs no table, and no transport
// registers it.
#include "rc_api_internal.h"

#include "rc_merge.h"

extern "C" {

int rc_read_merge_device(rc_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                         int32_t max_read_len, int32_t mode, const rc_merge_params *p, rc_read_merge *d_rows, uint8_t *d_mseq, uint8_t *d_mqual,
                         uint32_t *d_moff, uint64_t out_cap, rc_merge_tally *d_tally)
{
    if (!ctx) return RC_ERR_ARG;
    if (mode < 1 || mode > 2) {
        rc_set_error(ctx, "read_merge_device: mode %d (1 = pairs in two halves, 2 = interleaved pairs)", mode);
        return RC_ERR_ARG;
    }
    if (n_reads & 1u) {
        rc_set_error(ctx, "read_merge_device: pairs need an even number of reads (got %u)", n_reads);
        return RC_ERR_ARG;
    }
    if (!p) {
        rc_set_error(ctx, "read_merge_device: params must not be NULL");
        return RC_ERR_ARG;
    }
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "read_merge_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (max_read_len < 0 || max_read_len > RC_MERGE_MAX_LEN) {
        rc_set_error(ctx, "read_merge_device: max_read_len must be 0..%d (got %d)", RC_MERGE_MAX_LEN, max_read_len);
        return RC_ERR_ARG;
    }
    if (p->min_overlap < 1 || p->min_overlap > RC_MERGE_MAX_LEN) {
        rc_set_error(ctx, "read_merge_device: min_overlap must be 1..%d (got %d)", RC_MERGE_MAX_LEN, p->min_overlap);
        return RC_ERR_ARG;
    }
    if (p->max_mismatch_pct < 0 || p->max_mismatch_pct > 50) {
        rc_set_error(ctx, "read_merge_device: max_mismatch_pct must be 0..50 (got %d)", p->max_mismatch_pct);
        return RC_ERR_ARG;
    }
    if (p->qual_base < 0 || p->qual_base > 124) {
        rc_set_error(ctx, "read_merge_device: qual_base must be 0..124 (got %d)", p->qual_base);
        return RC_ERR_ARG;
    }
    if (p->qual_cap < 2 || p->qual_cap > 93) {
        rc_set_error(ctx, "read_merge_device: qual_cap must be 2..93 (got %d)", p->qual_cap);
        return RC_ERR_ARG;
    }
    if (p->qual_base + p->qual_cap > 126) {
        rc_set_error(ctx, "read_merge_device: qual_base + qual_cap must be at most 126 (got %d)", p->qual_base + p->qual_cap);
        return RC_ERR_ARG;
    }
    if (d_mqual && !d_qual) {
        rc_set_error(ctx, "read_merge_device: d_mqual given without d_qual: there are no qualities to merge");
        return RC_ERR_ARG;
    }
    if (out_cap < nbytes) {
        rc_set_error(ctx, "read_merge_device: out_cap of %llu bytes is below the input arena's %llu", (unsigned long long)out_cap, (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (n_reads && (!d_seq || !d_off || !d_rows || !d_mseq || !d_moff)) {  // (d_qual, d_mqual and d_tally may be NULL)
        rc_set_error(ctx, "read_merge_device: null pointer");
        return RC_ERR_ARG;
    }
    // (the kernels' 32-bit stores, 16-byte stores and 64-bit atomics)
    if (n_reads && (((uintptr_t)d_rows & 3u) || ((uintptr_t)d_moff & 3u) || ((uintptr_t)d_mseq & 15u) || ((uintptr_t)d_mqual & 15u) || ((uintptr_t)d_tally & 7u))) {
        rc_set_error(ctx, "read_merge_device: d_rows and d_moff must lie on a 4-byte boundary, d_mseq and d_mqual on a 16-byte one and d_tally on an 8-byte one");
        return RC_ERR_ARG;
    }
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_read_merge(ctx, d_seq, d_qual, (size_t)nbytes, d_off, n_reads, max_read_len, mode, p, d_rows, d_mseq, d_mqual, d_moff, (size_t)out_cap,
                                d_tally);
}

}  // extern "C"
