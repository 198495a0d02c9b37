// rc_api_depth.hip -- C ABI, the per-read k-mer depth (include/rcorrector_amd.h: rc_read_depth; kernel in rc_depth.hip): the
// device entry point and the one-shot registration of the slot transports.  What a registration leads to -- the kernel behind
// a batch's last correction kernel, the 16 bytes per read on the download stream -- is rc_api_slots.hip's, on the path the
// weak-k-mer profile's registration takes.
#include "rc_api_internal.h"

extern "C" {

int rc_read_depth_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes, int32_t max_read_len,
                         rc_read_depth *d_out)
{
    if (!ctx) return RC_ERR_ARG;
    if (n_reads && (!d_seq || !d_off || !d_out)) {
        rc_set_error(ctx, "read_depth_device: null pointer");
        return RC_ERR_ARG;
    }
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "read_depth_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (max_read_len >= RC_MAX_READ_LENGTH) {  // (what rc_launch_correct refuses; the kernel checks every read's length itself)
        rc_set_error(ctx, "read_depth_device: read of %d bases exceeds the %d-base limit (utils.h:7)", max_read_len, RC_MAX_READ_LENGTH - 1);
        return RC_ERR_ARG;
    }
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "read_depth: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    static_assert(sizeof(rc_read_depth) == 16, "16 bytes per read");
    return rc_launch_read_depth(ctx, d_seq, (size_t)nbytes, d_off, n_reads, d_out);
}

int rc_read_depth_into(rc_ctx *ctx, int slot, rc_read_depth *out)
{
    if (!ctx) return RC_ERR_ARG;
    if (slot < 0 || slot >= RC_MAX_SLOTS) {
        rc_set_error(ctx, "read_depth_into: no slot %d (0 .. %d)", slot, RC_MAX_SLOTS - 1);
        return RC_ERR_ARG;
    }
    if (out && !ctx->d_buckets) {
        rc_set_error(ctx, "read_depth: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    ctx->depth_reg[slot].out = out;
    return RC_OK;
}

}  // extern "C"
