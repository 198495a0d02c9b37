// rc_api_norm.hip -- C ABI, normalisation by k-mer depth (include/rcorrector_amd.h: rc_norm_select_device; the contract in
// rc_norm.h, the kernel in rc_norm.hip): the device entry point.  The selection reads depths, not reads: it needs no table, and
// no transport registers it.
#include "rc_api_internal.h"

extern "C" {

int rc_norm_select_device(rc_ctx *ctx, const rc_read_depth *d_depth, uint32_t n_units, int mode, uint64_t unit_base, uint32_t target, uint32_t min_cov,
                          uint64_t seed, uint32_t max_bin, uint8_t *d_keep, uint64_t *d_tally)
{
    if (!ctx) return RC_ERR_ARG;
    if (mode < 0 || mode > 2) {
        rc_set_error(ctx, "norm_select_device: mode %d (0 = reads, 1 = pairs in two halves, 2 = interleaved pairs)", mode);
        return RC_ERR_ARG;
    }
    if (target == 0 || target >= (1u << 31)) {
        rc_set_error(ctx, "norm_select_device: target = %u, must be 1 .. 2^31 - 1", target);
        return RC_ERR_ARG;
    }
    if (max_bin < 1 || max_bin > 65535) {
        rc_set_error(ctx, "norm_select_device: max_bin = %u, must be 1 .. 65535", max_bin);
        return RC_ERR_ARG;
    }
    if (n_units && (!d_depth || !d_keep || !d_tally)) {
        rc_set_error(ctx, "norm_select_device: null pointer");
        return RC_ERR_ARG;
    }
    if (n_units && (((uintptr_t)d_depth & 15u) || ((uintptr_t)d_tally & 7u))) {  // (the kernel's 16-byte loads and 64-bit atomics)
        rc_set_error(ctx, "norm_select_device: d_depth must lie on a 16-byte boundary and d_tally on an 8-byte one");
        return RC_ERR_ARG;
    }
    if (n_units == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    static_assert(sizeof(rc_read_depth) == 16, "16 bytes per read");
    return rc_launch_norm_select(ctx, d_depth, n_units, mode, unit_base, target, min_cov, seed, max_bin, d_keep, d_tally);
}

}  // extern "C"
