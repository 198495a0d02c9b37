// rc_api_trim.hip -- C ABI, read trimming (include/rcorrector_amd.h: rc_read_trim_device; the contract in rc_trim.h, the kernel in
// rc_trim.hip): the device entry point.  The cuts read bases and qualities, not k-mers: it needs no table, and no transport
// registers it.
#include "rc_api_internal.h"

#include "rc_trim.h"

static int trim_check_adapter(rc_ctx *ctx, const char *name, const uint8_t *ad, int32_t n)
{
    if (n < 0 || n > RC_TRIM_AD_MAX) {
        rc_set_error(ctx, "read_trim_device: %s_len must be 0..%d (got %d)", name, RC_TRIM_AD_MAX, n);
        return RC_ERR_ARG;
    }
    for (int i = 0; i < n; ++i)
        if (ad[i] != 'A' && ad[i] != 'C' && ad[i] != 'G' && ad[i] != 'T') {
            rc_set_error(ctx, "read_trim_device: %s holds a base outside upper-case ACGT at position %d (byte %d)", name, i, (int)ad[i]);
            return RC_ERR_ARG;
        }
    return RC_OK;
}

extern "C" {

int rc_read_trim_device(rc_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                        int32_t max_read_len, int32_t mode, const rc_trim_params *p, rc_read_trim *d_out, uint8_t *d_keep, rc_trim_tally *d_tally)
{
    if (!ctx) return RC_ERR_ARG;
    if (mode < 0 || mode > 2) {
        rc_set_error(ctx, "read_trim_device: mode %d (0 = reads, 1 = pairs in two halves, 2 = interleaved pairs)", mode);
        return RC_ERR_ARG;
    }
    if (mode != 0 && (n_reads & 1u)) {
        rc_set_error(ctx, "read_trim_device: pairs need an even number of reads (got %u)", n_reads);
        return RC_ERR_ARG;
    }
    if (!p) {
        rc_set_error(ctx, "read_trim_device: params must not be NULL");
        return RC_ERR_ARG;
    }
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "read_trim_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (max_read_len < 0 || max_read_len > RC_TRIM_MAX_LEN) {
        rc_set_error(ctx, "read_trim_device: max_read_len must be 0..%d (got %d)", RC_TRIM_MAX_LEN, max_read_len);
        return RC_ERR_ARG;
    }
    if (p->qual_min < 0 || p->qual_min > 93) {
        rc_set_error(ctx, "read_trim_device: qual_min must be 0..93 (got %d)", p->qual_min);
        return RC_ERR_ARG;
    }
    if (p->qual_base < 0 || p->qual_base > 255) {
        rc_set_error(ctx, "read_trim_device: qual_base must be 0..255 (got %d)", p->qual_base);
        return RC_ERR_ARG;
    }
    if (p->adapter_min < 1 || p->adapter_min > RC_TRIM_AD_MAX) {
        rc_set_error(ctx, "read_trim_device: adapter_min must be 1..%d (got %d)", RC_TRIM_AD_MAX, p->adapter_min);
        return RC_ERR_ARG;
    }
    if (p->adapter_mm_pct < 0 || p->adapter_mm_pct > 50) {
        rc_set_error(ctx, "read_trim_device: adapter_mm_pct must be 0..50 (got %d)", p->adapter_mm_pct);
        return RC_ERR_ARG;
    }
    if (p->pair_min_overlap < 1 || p->pair_min_overlap > RC_TRIM_MAX_LEN) {
        rc_set_error(ctx, "read_trim_device: pair_min_overlap must be 1..%d (got %d)", RC_TRIM_MAX_LEN, p->pair_min_overlap);
        return RC_ERR_ARG;
    }
    if (p->pair_mm_pct < 0 || p->pair_mm_pct > 50) {
        rc_set_error(ctx, "read_trim_device: pair_mm_pct must be 0..50 (got %d)", p->pair_mm_pct);
        return RC_ERR_ARG;
    }
    if (p->min_len < 0 || p->min_len > RC_TRIM_MAX_LEN) {
        rc_set_error(ctx, "read_trim_device: min_len must be 0..%d (got %d)", RC_TRIM_MAX_LEN, p->min_len);
        return RC_ERR_ARG;
    }
    if (const int rc = trim_check_adapter(ctx, "adapter1", p->adapter1, p->adapter1_len)) return rc;
    if (const int rc = trim_check_adapter(ctx, "adapter2", p->adapter2, p->adapter2_len)) return rc;
    if (n_reads && (!d_seq || !d_off || !d_out)) {  // (d_qual, d_keep and d_tally may be NULL)
        rc_set_error(ctx, "read_trim_device: null pointer");
        return RC_ERR_ARG;
    }
    if (n_reads && (((uintptr_t)d_out & 3u) || ((uintptr_t)d_tally & 7u))) {  // (the kernel's 32-bit stores and 64-bit atomics)
        rc_set_error(ctx, "read_trim_device: d_out must lie on a 4-byte boundary and d_tally on an 8-byte one");
        return RC_ERR_ARG;
    }
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_read_trim(ctx, d_seq, d_qual, (size_t)nbytes, d_off, n_reads, max_read_len, mode, p, d_out, d_keep, d_tally);
}

}  // extern "C"
