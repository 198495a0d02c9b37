// rc_api_dups.hip -- C ABI, the duplicate census (include/rcorrector_amd.h: rc_dup_census; kernels in rc_dups.hip): opening,
// reading, merging and closing it, and the two steps the correction entry points take for it.
//
// Where the keys go: a batch's BEFORE keys are taken on the stream of the context it runs in once its bases are in HBM and
// before the first correction kernel, its AFTER keys behind the last one (rc_dups_stage), both into scratch of the slot (or of
// the context, for the entry points that have no slot).  They reach the census when the batch completes (rc_dups_commit)
// -- once, however often a batch that did not fit its fix list was submitted.  Both steps are called from one place each,
// rc_correct_observed and rc_batch_completed (rc_api_observe.hip), which say where they sit for every entry point.  Slot lanes
// are contexts on streams of their own: they append to the census of the context they serve under its obs_mutex.  A commit is
// complete on return, so the accumulators can be moved when they grow; a growth that fails fails the call that completes the
// batch with RC_STATUS_NOSPACE.
#include "rc_api_internal.h"

#define RC_DUP_MAX_BIN (1u << 28)

extern "C" {

int rc_dups_stage(rc_ctx *ctx, const rc_device_batch *b, int version, rc_batch_observed *o)
{
    rc_ctx *home = rc_home(ctx);
    if (version == 0) {
        o->dup_units = 0;
        if (!home->dup_open) return RC_OK;
        const size_t n = b->mode == 0 ? b->n_reads : b->n_reads >> 1;
        if (!n) return RC_OK;
        if (const int rc = rc_dbuf_reserve(ctx, &o->dup_keys, 2 * n * 16)) return rc;
        if (const int rc = rc_launch_read_keys(ctx, ctx->stream, b->d_seq, (size_t)b->nbytes, b->d_off, b->n_reads, b->mode, (uint64_t *)o->dup_keys.p)) return rc;
        o->dup_units = n;
        o->dup_gen = home->dup_gen;
        return RC_OK;
    }
    if (!o->dup_units) return RC_OK;  // (no census was open when the batch's bases arrived: it is in none)
    return rc_launch_read_keys(ctx, ctx->stream, b->d_seq, (size_t)b->nbytes, b->d_off, b->n_reads, b->mode, (uint64_t *)o->dup_keys.p + 2 * o->dup_units);
}

// room for `more` units behind home's dup_n; called with obs_mutex held and nothing outstanding on the accumulators
static int dups_grow(rc_ctx *err_ctx, rc_ctx *home, size_t more)
{
    const size_t need = home->dup_n + more;
    if (need >= (1ull << 32)) {
        rc_set_error(err_ctx, "dup census: %zu units are more than a census holds (2^32 - 1)", need);
        return RC_ERR_NOSPACE;
    }
    if (need <= home->dup_cap) return RC_OK;
    const size_t cap = std::max(std::max(need, home->dup_cap * 2), (size_t)1 << 16);
    void *nw[2] = {nullptr, nullptr};
    for (int v = 0; v < 2; ++v) {
        if (hipMalloc(&nw[v], cap * 16) != hipSuccess) {
            (void)hipGetLastError();
            if (nw[0]) (void)hipFree(nw[0]);
            rc_set_error(err_ctx, "dup census: no device memory for the keys of %zu units (2 x %zu MB): the census would be short", need, (cap * 16) >> 20);
            return RC_ERR_NOSPACE;
        }
    }
    for (int v = 0; v < 2; ++v) {
        if (home->dup_n && hipMemcpy(nw[v], home->dup_acc[v], home->dup_n * 16, hipMemcpyDeviceToDevice) != hipSuccess) {
            (void)hipFree(nw[0]);
            (void)hipFree(nw[1]);
            rc_set_error(err_ctx, "dup census: could not move the keys");
            return RC_ERR_HIP;
        }
    }
    for (int v = 0; v < 2; ++v) {
        if (home->dup_acc[v]) (void)hipFree(home->dup_acc[v]);
        home->dup_acc[v] = nw[v];
    }
    home->dup_cap = cap;
    return RC_OK;
}

int rc_dups_commit(rc_ctx *ctx, rc_batch_observed *o)
{
    const size_t n = o->dup_units;
    o->dup_units = 0;
    if (!n) return RC_OK;
    rc_ctx *home = rc_home(ctx);
    int rc = RC_OK;
    {
        std::lock_guard<std::mutex> lk(home->obs_mutex);
        if (!home->dup_open || home->dup_gen != o->dup_gen) return RC_OK;  // (staged for a census that has ended)
        if (!(rc = dups_grow(ctx, home, n))) {
            const char *src = (const char *)o->dup_keys.p;
            hipError_t e = hipMemcpyAsync((char *)home->dup_acc[0] + home->dup_n * 16, src, n * 16, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess) e = hipMemcpyAsync((char *)home->dup_acc[1] + home->dup_n * 16, src + n * 16, n * 16, hipMemcpyDeviceToDevice, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e != hipSuccess) {
                rc_set_error(ctx, "dup census: appending %zu keys failed: %s", n, hipGetErrorString(e));
                rc = RC_ERR_HIP;
            } else {
                home->dup_n += n;
            }
        }
    }
    return rc;
}

static void dups_release(rc_ctx *ctx)
{
    for (int v = 0; v < 2; ++v) {
        if (ctx->dup_acc[v]) (void)hipFree(ctx->dup_acc[v]);
        ctx->dup_acc[v] = nullptr;
    }
    ctx->dup_n = ctx->dup_cap = 0;
    ctx->dup_open = false;
    rc_observed_drop_all(ctx, RC_OBS_DUPS, true);  // (the staged keys of ctx, its lanes and their slots)
}

int rc_dup_census_begin(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    if (ctx->dup_open) {
        rc_set_error(ctx, "dup_census_begin: a census is open already (rc_dup_census_end it first)");
        return RC_ERR_STATE;
    }
    ctx->dup_n = 0;
    ++ctx->dup_gen;
    ctx->dup_open = true;
    return RC_OK;
}

int rc_dup_census_get(rc_ctx *ctx, uint32_t max_bin, rc_dup_census *out)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->dup_open) {
        rc_set_error(ctx, "dup_census_get: call rc_dup_census_begin first");
        return RC_ERR_STATE;
    }
    if (!out || !out->copies_before || !out->copies_after || max_bin < 1 || max_bin > RC_DUP_MAX_BIN) {
        rc_set_error(ctx, "dup_census_get: max_bin must be 1..%u, out and its two arrays not NULL", RC_DUP_MAX_BIN);
        return RC_ERR_ARG;
    }
    if (const int rc = rc_drain(ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    out->units = ctx->dup_n;
    if (const int rc = rc_dup_census_run(ctx, (const uint64_t *)ctx->dup_acc[0], ctx->dup_n, max_bin, out->copies_before, &out->distinct_before)) return rc;
    return rc_dup_census_run(ctx, (const uint64_t *)ctx->dup_acc[1], ctx->dup_n, max_bin, out->copies_after, &out->distinct_after);
}

int rc_dup_census_end(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->dup_open) {
        rc_set_error(ctx, "dup_census_end: no census is open");
        return RC_ERR_STATE;
    }
    const int rc = rc_drain(ctx);  // (a lane's key kernels may still write its slot's scratch)
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    dups_release(ctx);
    return rc;
}

int rc_read_keys_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes, int mode, uint64_t *d_keys)
{
    if (!ctx) return RC_ERR_ARG;
    if (mode < 0 || mode > 2) {
        rc_set_error(ctx, "read_keys_device: mode must be 0, 1 or 2 (got %d)", mode);
        return RC_ERR_ARG;
    }
    if (mode != 0 && (n_reads & 1u)) {
        rc_set_error(ctx, "read_keys_device: %s mode needs an even number of reads (got %u)", mode == 1 ? "paired" : "interleaved", n_reads);
        return RC_ERR_ARG;
    }
    if (n_reads && (!d_seq || !d_off || !d_keys)) {
        rc_set_error(ctx, "read_keys_device: null pointer");
        return RC_ERR_ARG;
    }
    if ((uintptr_t)d_keys & 15u) {
        rc_set_error(ctx, "read_keys_device: d_keys must be 16-byte aligned");
        return RC_ERR_ARG;
    }
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "read_keys_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_read_keys(ctx, ctx->stream, d_seq, (size_t)nbytes, d_off, n_reads, mode, d_keys);
}

int rc_dup_census_merge(rc_ctx *dst, rc_ctx *src)
{
    if (!dst || !src) return RC_ERR_ARG;
    if (dst == src) {
        rc_set_error(dst, "dup_census_merge: a census cannot be merged into itself");
        return RC_ERR_ARG;
    }
    if (!dst->dup_open || !src->dup_open) {
        rc_set_error(dst, "dup_census_merge: both contexts need an open census (rc_dup_census_begin)");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(dst, hipSetDevice(src->device));
    if (rc_drain(src)) {
        rc_set_error(dst, "dup_census_merge: the source context's work did not complete: %s", rc_last_error(src));
        return RC_ERR_HIP;
    }
    if (const int rc = rc_drain(dst)) return rc;  // (and dst's device is current again)
    std::lock(dst->obs_mutex, src->obs_mutex);
    std::lock_guard<std::mutex> l1(dst->obs_mutex, std::adopt_lock), l2(src->obs_mutex, std::adopt_lock);
    const size_t n = src->dup_n;
    if (!n) return RC_OK;
    if (const int rc = dups_grow(dst, dst, n)) return rc;
    for (int v = 0; v < 2; ++v) {
        char *to = (char *)dst->dup_acc[v] + dst->dup_n * 16;
        hipError_t e = dst->device == src->device ? hipMemcpy(to, src->dup_acc[v], n * 16, hipMemcpyDeviceToDevice)
                                                  : hipMemcpyPeer(to, dst->device, src->dup_acc[v], src->device, n * 16);
        if (e != hipSuccess) {  // no way between the two devices: through the host
            (void)hipGetLastError();
            std::vector<char> h(n * 16);
            RC_CHECK_HIP(dst, hipSetDevice(src->device));
            RC_CHECK_HIP(dst, hipMemcpy(h.data(), src->dup_acc[v], n * 16, hipMemcpyDeviceToHost));
            RC_CHECK_HIP(dst, hipSetDevice(dst->device));
            RC_CHECK_HIP(dst, hipMemcpy(to, h.data(), n * 16, hipMemcpyHostToDevice));
        }
    }
    dst->dup_n += n;
    return RC_OK;
}

}  // extern "C"
