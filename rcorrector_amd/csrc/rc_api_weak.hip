// rc_api_weak.hip -- C ABI, the per-read weak-k-mer profile (include/rcorrector_amd.h: rc_read_weak; kernels in rc_weak.hip):
// the device entry point and the one-shot registration of the slot transports.  What a registration leads to -- the kernels
// behind a batch's last correction kernel, the 16 bytes per read on the download stream -- is rc_api_slots.hip's
// (in_slot_lane takes the registration with the submit, slot_download consumes it, slot_results_back hands it over).
#include "rc_api_internal.h"

extern "C" {

int rc_weak_profile_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes, int32_t max_read_len,
                           int32_t min_count, rc_read_weak *d_out)
{
    if (!ctx) return RC_ERR_ARG;
    if (min_count < 1) {
        rc_set_error(ctx, "weak_profile_device: min_count must be at least 1 (got %d)", min_count);
        return RC_ERR_ARG;
    }
    if (n_reads && (!d_seq || !d_off || !d_out)) {
        rc_set_error(ctx, "weak_profile_device: null pointer");
        return RC_ERR_ARG;
    }
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "weak_profile_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "weak_profile: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    (void)max_read_len;  // (the reduce takes a read of any length: one lane walks its plane words)
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    static_assert(sizeof(rc_read_weak) == 16, "16 bytes per read");
    return rc_launch_weak_profile(ctx, d_seq, (size_t)nbytes, d_off, n_reads, min_count, &ctx->weak_planes, d_out);
}

int rc_weak_profile_into(rc_ctx *ctx, int slot, rc_read_weak *out, int32_t min_count)
{
    if (!ctx) return RC_ERR_ARG;
    if (slot < 0 || slot >= RC_MAX_SLOTS) {
        rc_set_error(ctx, "weak_profile_into: no slot %d (0 .. %d)", slot, RC_MAX_SLOTS - 1);
        return RC_ERR_ARG;
    }
    if (out && min_count < 1) {
        rc_set_error(ctx, "weak_profile_into: min_count must be at least 1 (got %d)", min_count);
        return RC_ERR_ARG;
    }
    if (out && !ctx->d_buckets) {
        rc_set_error(ctx, "weak_profile: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    ctx->weak_reg[slot].out = out;
    ctx->weak_reg[slot].min_count = out ? min_count : 1;
    return RC_OK;
}

}  // extern "C"
