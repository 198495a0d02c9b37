// rc_api_screen.hip -- C ABI, the per-read hit profile against a second k-mer set (include/rcorrector_amd.h: rc_read_screen;
// kernel in rc_screen.hip): the device entry point and the one-shot registration of the slot transports.  What a registration
// leads to -- the kernel behind a batch's last correction kernel, the 16 bytes per read on the download stream -- is
// rc_api_slots.hip's, on the path the weak-k-mer profile's and the depth's registrations take.
#include "rc_api_internal.h"

// what both entry points ask of the screen context: a table of ctx's k on ctx's device
static int screen_table_fits(rc_ctx *ctx, const rc_ctx *screen, const char *name)
{
    if (screen->k != ctx->k) {
        rc_set_error(ctx, "%s: the screen table is of k = %d, the context of k = %d", name, screen->k, ctx->k);
        return RC_ERR_ARG;
    }
    if (screen->device != ctx->device) {
        rc_set_error(ctx, "%s: the screen table is on device %d, the context on device %d (rc_table_replicate brings a copy over)", name, screen->device,
                     ctx->device);
        return RC_ERR_ARG;
    }
    if (!screen->d_buckets) {
        rc_set_error(ctx, "%s: no k-mer table in the screen context", name);
        return RC_ERR_STATE;
    }
    return RC_OK;
}

extern "C" {

int rc_read_screen_device(rc_ctx *ctx, const rc_ctx *screen, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                          int32_t max_read_len, int32_t min_count, rc_read_screen *d_out)
{
    if (!ctx) return RC_ERR_ARG;
    if (!screen || (n_reads && (!d_seq || !d_off || !d_out))) {
        rc_set_error(ctx, "read_screen_device: null pointer");
        return RC_ERR_ARG;
    }
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "read_screen_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (max_read_len >= RC_MAX_READ_LENGTH) {  // (what rc_launch_correct refuses; the kernel checks every read's length itself)
        rc_set_error(ctx, "read_screen_device: read of %d bases exceeds the %d-base limit (utils.h:7)", max_read_len, RC_MAX_READ_LENGTH - 1);
        return RC_ERR_ARG;
    }
    if (min_count < 1) {
        rc_set_error(ctx, "read_screen_device: min_count = %d, must be at least 1", min_count);
        return RC_ERR_ARG;
    }
    if (const int rc = screen_table_fits(ctx, screen, "read_screen_device")) return rc;
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    static_assert(sizeof(rc_read_screen) == 16, "16 bytes per read");
    return rc_launch_read_screen(ctx, screen, d_seq, (size_t)nbytes, d_off, n_reads, min_count, d_out);
}

int rc_read_screen_into(rc_ctx *ctx, int slot, const rc_ctx *screen, int32_t min_count, rc_read_screen *out)
{
    if (!ctx) return RC_ERR_ARG;
    if (slot < 0 || slot >= RC_MAX_SLOTS) {
        rc_set_error(ctx, "read_screen_into: no slot %d (0 .. %d)", slot, RC_MAX_SLOTS - 1);
        return RC_ERR_ARG;
    }
    if (!out) {  // (withdrawn: neither the screen context nor min_count is looked at)
        ctx->screen_reg[slot] = rc_ctx::rc_screen_reg();
        return RC_OK;
    }
    if (!screen) {
        rc_set_error(ctx, "read_screen_into: null pointer");
        return RC_ERR_ARG;
    }
    if (min_count < 1) {
        rc_set_error(ctx, "read_screen_into: min_count = %d, must be at least 1", min_count);
        return RC_ERR_ARG;
    }
    if (const int rc = screen_table_fits(ctx, screen, "read_screen_into")) return rc;
    ctx->screen_reg[slot].out = out;
    ctx->screen_reg[slot].screen = screen;
    ctx->screen_reg[slot].min_count = min_count;
    return RC_OK;
}

}  // extern "C"
