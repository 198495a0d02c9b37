// rc_api_recur.hip -- C ABI, the recurrent-correction census (include/rcorrector_amd.h: rc_recur_census; kernels in
// rc_recur.hip): the device entry point, opening, reading, merging and closing a census, and the two steps the correction entry
// points take for it.
//
// Where the keys go: the kernel needs both versions of a batch at once, so it runs once, behind the batch's last correction
// kernel (rc_recur_stage), on the stream of the context the batch runs in: the arena as it arrived is the copy
// rc_report_snapshot took in front of the first correction kernel -- one copy, shared with the correction report and the
// mate-overlap session where several are open.  How many keys a batch has is not known ahead: the kernel appends into scratch of
// the slot (or of the context, for the entry points that have no slot) sized for one contexted change in 32 arena bytes, three
// times what a run at 1 % changed bases leaves, and counts exactly; the stage then WAITS for the stream, reads the three counts,
// and where the keys did not fit reserves what they need and launches once more -- the snapshot is still there, which it is not
// any more when the batch completes.  So a submit blocks until the batch's kernels have run while a census is open.  The keys
// reach the census when the batch completes (rc_recur_commit) -- once, however often a batch that did not fit its fix list was
// submitted.  Both steps are called from one place each, rc_correct_observed and rc_batch_completed (rc_api_observe.hip).  Slot
// lanes are contexts on streams of their own: they append to the census of the context they serve under its obs_mutex.  A commit
// is complete on return, so the accumulator can be moved when it grows; a growth that fails fails the call that completes the
// batch with RC_STATUS_NOSPACE.
#include "rc_api_internal.h"

#include "rc_recur.h"

#define RC_RECUR_MAX_BIN (1u << 28)

extern "C" {

int rc_recur_stage(rc_ctx *ctx, const rc_device_batch *b, const uint8_t *snap, rc_batch_observed *o)
{
    o->recur_staged = false;
    o->recur_n = o->recur_changes = o->recur_contexted = 0;
    rc_ctx *home = rc_home(ctx);
    // (snap == nullptr: no census was open when the batch's bases arrived -- it is in none)
    if (!home->recur_open || !snap || !b->n_reads) return RC_OK;
    o->recur_gen = home->recur_gen;
    if (const int rc = rc_dbuf_reserve(ctx, &o->recur_counts, 3 * sizeof(uint64_t))) return rc;
    uint64_t cap = std::max<uint64_t>((uint64_t)b->nbytes / 32, 4096);
    for (int pass = 0; pass < 2; ++pass) {
        if (const int rc = rc_dbuf_reserve(ctx, &o->recur_keys, (size_t)cap * 8)) return rc;
        if (const int rc = rc_launch_change_keys(ctx, ctx->stream, snap, b->d_seq, b->d_off, b->n_reads, (size_t)b->nbytes, (uint64_t *)o->recur_keys.p, cap,
                                                 (uint64_t *)o->recur_counts.p))
            return rc;
        uint64_t c[3];
        RC_CHECK_HIP(ctx, hipMemcpyAsync(c, o->recur_counts.p, sizeof c, hipMemcpyDeviceToHost, ctx->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        o->recur_changes = c[0];
        o->recur_contexted = c[1];
        o->recur_n = c[2];
        if (c[2] <= cap) break;
        if (pass) {
            rc_set_error(ctx, "recurrence census: internal: %llu keys where %llu were counted", (unsigned long long)c[2], (unsigned long long)cap);
            return RC_ERR_STATE;
        }
        cap = c[2];  // (they did not fit: once more, with room for exactly these)
    }
    o->recur_staged = true;
    return RC_OK;
}

// room for `more` keys behind home's recur_n; called with obs_mutex held and nothing outstanding on the accumulator
static int recur_grow(rc_ctx *err_ctx, rc_ctx *home, size_t more)
{
    const size_t need = home->recur_n + more;
    if (need >= (1ull << 32)) {
        rc_set_error(err_ctx, "recurrence census: %zu keys are more than a census holds (2^32 - 1)", need);
        return RC_ERR_NOSPACE;
    }
    if (need <= home->recur_cap) return RC_OK;
    const size_t cap = std::max(std::max(need, home->recur_cap * 2), (size_t)1 << 16);
    void *nw = nullptr;
    if (hipMalloc(&nw, cap * 8) != hipSuccess) {
        (void)hipGetLastError();
        rc_set_error(err_ctx, "recurrence census: no device memory for %zu keys (%zu MB): the census would be short", need, (cap * 8) >> 20);
        return RC_ERR_NOSPACE;
    }
    if (home->recur_n && hipMemcpy(nw, home->recur_acc, home->recur_n * 8, hipMemcpyDeviceToDevice) != hipSuccess) {
        (void)hipFree(nw);
        rc_set_error(err_ctx, "recurrence census: could not move the keys");
        return RC_ERR_HIP;
    }
    if (home->recur_acc) (void)hipFree(home->recur_acc);
    home->recur_acc = nw;
    home->recur_cap = cap;
    return RC_OK;
}

int rc_recur_commit(rc_ctx *ctx, rc_batch_observed *o)
{
    if (!o->recur_staged) return RC_OK;
    o->recur_staged = false;
    const size_t n = (size_t)o->recur_n;
    rc_ctx *home = rc_home(ctx);
    std::lock_guard<std::mutex> lk(home->obs_mutex);
    if (!home->recur_open || home->recur_gen != o->recur_gen) return RC_OK;  // (staged for a census that has ended)
    if (n) {
        if (const int rc = recur_grow(ctx, home, n)) return rc;
        hipError_t e = hipMemcpyAsync((char *)home->recur_acc + home->recur_n * 8, o->recur_keys.p, n * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) {
            rc_set_error(ctx, "recurrence census: appending %zu keys failed: %s", n, hipGetErrorString(e));
            return RC_ERR_HIP;
        }
        home->recur_n += n;
    }
    home->recur_changes += o->recur_changes;
    home->recur_contexted += o->recur_contexted;
    return RC_OK;
}

void rc_recur_release(rc_ctx *ctx)
{
    if (ctx->recur_acc) (void)hipFree(ctx->recur_acc);
    ctx->recur_acc = nullptr;
    ctx->recur_n = ctx->recur_cap = 0;
    ctx->recur_changes = ctx->recur_contexted = 0;
    ctx->recur_open = false;
}

int rc_recur_census_begin(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    if (ctx->recur_open) {
        rc_set_error(ctx, "recur_census_begin: a census is open already (rc_recur_census_end it first)");
        return RC_ERR_STATE;
    }
    ctx->recur_n = 0;
    ctx->recur_changes = ctx->recur_contexted = 0;
    ++ctx->recur_gen;
    ctx->recur_open = true;
    return RC_OK;
}

int rc_recur_census_get(rc_ctx *ctx, uint32_t max_bin, uint32_t min_count, uint32_t max_sites, rc_recur_census *out)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->recur_open) {
        rc_set_error(ctx, "recur_census_get: call rc_recur_census_begin first");
        return RC_ERR_STATE;
    }
    if (!out || !out->recur || (max_sites && (!out->top_key || !out->top_count)) || max_bin < 1 || max_bin > RC_RECUR_MAX_BIN || min_count < 1) {
        rc_set_error(ctx, "recur_census_get: max_bin must be 1..%u, min_count at least 1, out and its arrays not NULL", RC_RECUR_MAX_BIN);
        return RC_ERR_ARG;
    }
    if (const int rc = rc_drain(ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    out->changes = ctx->recur_changes;
    out->contexted = ctx->recur_contexted;
    out->clipped = ctx->recur_changes - ctx->recur_contexted;
    return rc_recur_census_run(ctx, (const uint64_t *)ctx->recur_acc, ctx->recur_n, max_bin, min_count, max_sites, out->recur, &out->sites, &out->sites_recurrent,
                               &out->changes_at_recurrent, out->top_key, out->top_count, &out->n_top);
}

int rc_recur_census_end(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->recur_open) {
        rc_set_error(ctx, "recur_census_end: no census is open");
        return RC_ERR_STATE;
    }
    const int rc = rc_drain(ctx);  // (a lane's key kernel may still write its slot's scratch)
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    rc_recur_release(ctx);
    rc_observed_drop_all(ctx, RC_OBS_RECUR, true);  // (the staged keys of ctx, its lanes and their slots)
    return rc;
}

int rc_change_keys_device(rc_ctx *ctx, const uint8_t *d_before, const uint8_t *d_after, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                          uint64_t *d_keys, uint64_t cap, uint64_t *d_counts)
{
    if (!ctx) return RC_ERR_ARG;
    if (!d_counts || (n_reads && (!d_before || !d_after || !d_off)) || (cap && !d_keys)) {
        rc_set_error(ctx, "change_keys_device: null pointer");
        return RC_ERR_ARG;
    }
    if (((uintptr_t)d_keys & 7u) || ((uintptr_t)d_counts & 7u)) {
        rc_set_error(ctx, "change_keys_device: d_keys and d_counts must be 8-byte aligned");
        return RC_ERR_ARG;
    }
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "change_keys_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (n_reads && (((uintptr_t)d_before ^ (uintptr_t)d_after) & 15u)) {
        rc_set_error(ctx, "change_keys_device: d_before and d_after must have the same alignment modulo 16");
        return RC_ERR_ARG;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_change_keys(ctx, ctx->stream, d_before, d_after, d_off, n_reads, (size_t)nbytes, d_keys, cap, d_counts);
}

int rc_recur_census_merge(rc_ctx *dst, rc_ctx *src)
{
    if (!dst || !src) return RC_ERR_ARG;
    if (dst == src) {
        rc_set_error(dst, "recur_census_merge: a census cannot be merged into itself");
        return RC_ERR_ARG;
    }
    if (!dst->recur_open || !src->recur_open) {
        rc_set_error(dst, "recur_census_merge: both contexts need an open census (rc_recur_census_begin)");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(dst, hipSetDevice(src->device));
    if (rc_drain(src)) {
        rc_set_error(dst, "recur_census_merge: the source context's work did not complete: %s", rc_last_error(src));
        return RC_ERR_HIP;
    }
    if (const int rc = rc_drain(dst)) return rc;  // (and dst's device is current again)
    std::lock(dst->obs_mutex, src->obs_mutex);
    std::lock_guard<std::mutex> l1(dst->obs_mutex, std::adopt_lock), l2(src->obs_mutex, std::adopt_lock);
    const size_t n = src->recur_n;
    if (n) {
        if (const int rc = recur_grow(dst, dst, n)) return rc;
        char *to = (char *)dst->recur_acc + dst->recur_n * 8;
        hipError_t e = dst->device == src->device ? hipMemcpy(to, src->recur_acc, n * 8, hipMemcpyDeviceToDevice)
                                                  : hipMemcpyPeer(to, dst->device, src->recur_acc, src->device, n * 8);
        if (e != hipSuccess) {  // no way between the two devices: through the host
            (void)hipGetLastError();
            std::vector<char> h(n * 8);
            RC_CHECK_HIP(dst, hipSetDevice(src->device));
            RC_CHECK_HIP(dst, hipMemcpy(h.data(), src->recur_acc, n * 8, hipMemcpyDeviceToHost));
            RC_CHECK_HIP(dst, hipSetDevice(dst->device));
            RC_CHECK_HIP(dst, hipMemcpy(to, h.data(), n * 8, hipMemcpyHostToDevice));
        }
        dst->recur_n += n;
    }
    dst->recur_changes += src->recur_changes;
    dst->recur_contexted += src->recur_contexted;
    return RC_OK;
}

}  // extern "C"
