// rc_api_payload.hip -- C ABI, the three per-read payloads, 16 bytes per read each (include/rcorrector_amd.h): the weak-k-mer
// profile (rc_read_weak; kernels in rc_weak.hip), the k-mer depth (rc_read_depth; kernel in rc_depth.hip) and the hit profile
// against a second k-mer set (rc_read_screen; kernel in rc_screen.hip) -- of each the device entry point and the one-shot
// registration of the slot transports.  What a registration leads to -- the kernels behind a batch's last correction kernel,
// the 16 bytes per read on the download stream -- is rc_api_slots.hip's (in_slot_lane takes the registrations with the submit,
// slot_download consumes them, slot_results_back hands the values over).
#include "rc_api_internal.h"

static_assert(sizeof(rc_read_weak) == 16 && sizeof(rc_read_depth) == 16 && sizeof(rc_read_screen) == 16, "16 bytes per read");

// ---- the refusals the entry points share, in `name`'s words; each entry point calls them in its own order -----------------
static int slot_exists(rc_ctx *ctx, const char *name, int slot)
{
    if (slot >= 0 && slot < RC_MAX_SLOTS) return RC_OK;
    rc_set_error(ctx, "%s: no slot %d (0 .. %d)", name, slot, RC_MAX_SLOTS - 1);
    return RC_ERR_ARG;
}

static int pointers_given(rc_ctx *ctx, const char *name, bool given)
{
    if (given) return RC_OK;
    rc_set_error(ctx, "%s: null pointer", name);
    return RC_ERR_ARG;
}

static int arena_fits(rc_ctx *ctx, const char *name, uint64_t nbytes)
{
    if (nbytes < (1ull << 32)) return RC_OK;
    rc_set_error(ctx, "%s: arena of %llu bytes exceeds the 4 GiB batch limit", name, (unsigned long long)nbytes);
    return RC_ERR_ARG;
}

// (what rc_launch_correct refuses; the kernels check every read's length themselves)
static int reads_fit(rc_ctx *ctx, const char *name, int32_t max_read_len)
{
    if (max_read_len < RC_MAX_READ_LENGTH) return RC_OK;
    rc_set_error(ctx, "%s: read of %d bases exceeds the %d-base limit (utils.h:7)", name, max_read_len, RC_MAX_READ_LENGTH - 1);
    return RC_ERR_ARG;
}

// fmt: the payload's spelling of the refusal, over (name, min_count)
static int min_count_fits(rc_ctx *ctx, const char *name, int32_t min_count, const char *fmt)
{
    if (min_count >= 1) return RC_OK;
    rc_set_error(ctx, fmt, name, min_count);
    return RC_ERR_ARG;
}
#define WEAK_MIN_COUNT "%s: min_count must be at least 1 (got %d)"
#define SCREEN_MIN_COUNT "%s: min_count = %d, must be at least 1"

// what: the payload, not the entry point
static int table_loaded(rc_ctx *ctx, const char *what)
{
    if (ctx->d_buckets) return RC_OK;
    rc_set_error(ctx, "%s: no k-mer table loaded", what);
    return RC_ERR_STATE;
}

// what both screen entry points ask of the screen context: a table of ctx's k on ctx's device
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

// a registration into its place in the table; out == nullptr withdraws it, whatever else the caller passed
static int payload_register(rc_ctx *ctx, int kind, int slot, void *out, int32_t min_count, const rc_ctx *screen)
{
    rc_ctx::rc_payload_reg reg;
    if (out) {
        reg.out = out;
        reg.min_count = min_count;
        reg.screen = screen;
    }
    ctx->payload_reg[kind][slot] = reg;
    return RC_OK;
}

extern "C" {

int rc_weak_profile_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes, int32_t max_read_len,
                           int32_t min_count, rc_read_weak *d_out)
{
    const char *name = "weak_profile_device";
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = min_count_fits(ctx, name, min_count, WEAK_MIN_COUNT)) return rc;
    if (const int rc = pointers_given(ctx, name, !n_reads || (d_seq && d_off && d_out))) return rc;
    if (const int rc = arena_fits(ctx, name, nbytes)) return rc;
    if (const int rc = table_loaded(ctx, "weak_profile")) return rc;
    (void)max_read_len;  // (the reduce takes a read of any length: one lane walks its plane words)
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_weak_profile(ctx, d_seq, (size_t)nbytes, d_off, n_reads, min_count, &ctx->weak_planes, d_out);
}

int rc_weak_profile_into(rc_ctx *ctx, int slot, rc_read_weak *out, int32_t min_count)
{
    const char *name = "weak_profile_into";
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = slot_exists(ctx, name, slot)) return rc;
    if (out) {
        if (const int rc = min_count_fits(ctx, name, min_count, WEAK_MIN_COUNT)) return rc;
        if (const int rc = table_loaded(ctx, "weak_profile")) return rc;
    }
    return payload_register(ctx, RC_PAY_WEAK, slot, out, min_count, nullptr);
}

int rc_read_depth_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes, int32_t max_read_len,
                         rc_read_depth *d_out)
{
    const char *name = "read_depth_device";
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = pointers_given(ctx, name, !n_reads || (d_seq && d_off && d_out))) return rc;
    if (const int rc = arena_fits(ctx, name, nbytes)) return rc;
    if (const int rc = reads_fit(ctx, name, max_read_len)) return rc;
    if (const int rc = table_loaded(ctx, "read_depth")) return rc;
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_read_depth(ctx, d_seq, (size_t)nbytes, d_off, n_reads, d_out);
}

int rc_read_depth_into(rc_ctx *ctx, int slot, rc_read_depth *out)
{
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = slot_exists(ctx, "read_depth_into", slot)) return rc;
    if (out)
        if (const int rc = table_loaded(ctx, "read_depth")) return rc;
    return payload_register(ctx, RC_PAY_DEPTH, slot, out, 1, nullptr);
}

int rc_read_screen_device(rc_ctx *ctx, const rc_ctx *screen, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                          int32_t max_read_len, int32_t min_count, rc_read_screen *d_out)
{
    const char *name = "read_screen_device";
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = pointers_given(ctx, name, screen && (!n_reads || (d_seq && d_off && d_out)))) return rc;
    if (const int rc = arena_fits(ctx, name, nbytes)) return rc;
    if (const int rc = reads_fit(ctx, name, max_read_len)) return rc;
    if (const int rc = min_count_fits(ctx, name, min_count, SCREEN_MIN_COUNT)) return rc;
    if (const int rc = screen_table_fits(ctx, screen, name)) return rc;
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_read_screen(ctx, screen, d_seq, (size_t)nbytes, d_off, n_reads, min_count, d_out);
}

int rc_read_screen_into(rc_ctx *ctx, int slot, const rc_ctx *screen, int32_t min_count, rc_read_screen *out)
{
    const char *name = "read_screen_into";
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = slot_exists(ctx, name, slot)) return rc;
    if (out) {  // (withdrawn: neither the screen context nor min_count is looked at)
        if (const int rc = pointers_given(ctx, name, screen)) return rc;
        if (const int rc = min_count_fits(ctx, name, min_count, SCREEN_MIN_COUNT)) return rc;
        if (const int rc = screen_table_fits(ctx, screen, name)) return rc;
    }
    return payload_register(ctx, RC_PAY_SCREEN, slot, out, min_count, screen);
}

}  // extern "C"
