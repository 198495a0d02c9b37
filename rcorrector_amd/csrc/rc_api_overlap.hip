// rc_api_overlap.hip -- C ABI, the mate-overlap report (include/rcorrector_amd.h: rc_mate_overlap; kernel in rc_overlap.hip): the
// device entry point, opening, reading and closing a session, and the two steps the correction entry points take for it.
//
// Where the counts go: the kernel needs both versions of a batch at once, so it runs once, behind the batch's last correction
// kernel (rc_overlap_stage), on the stream of the context the batch runs in: the arena as it arrived is the copy
// rc_report_snapshot took in front of the first correction kernel -- one copy, shared with the correction report where both are
// open -- and the arena as corrected is the batch's own.  It counts into an rc_mate_overlap of the slot (or of the context, for
// the entry points that have no slot), zeroed first, which is added to the session when the batch completes
// (rc_overlap_commit) -- once, however often a batch that did not fit its fix list was submitted.  Both steps are called from
// one place each, rc_correct_observed and rc_batch_completed (rc_api_observe.hip).  Slot lanes are contexts on streams of their
// own: they add to the session of the context they serve under its obs_mutex, and a commit is complete on return, so two lanes
// never add at once and a slot's block is free again.  A single-end batch has no pairs: it stages nothing.
#include "rc_api_internal.h"

#include <cstddef>

#include "rc_overlap.h"

#define RC_OVL_WORDS (sizeof(rc_mate_overlap) / 8)
static_assert(offsetof(rc_mate_overlap, pairs) == 16 && offsetof(rc_mate_overlap, frag) == 14 * 8 &&
                  offsetof(rc_mate_overlap, compared5) == (14 + RC_OV_FRAG) * 8 &&
                  offsetof(rc_mate_overlap, disagree5_before) == (14 + RC_OV_FRAG + 2 * RC_OV_POS) * 8 &&
                  offsetof(rc_mate_overlap, disagree5_after) == (14 + RC_OV_FRAG + 4 * RC_OV_POS) * 8,
              "two parameters, twelve totals, frag, compared5, disagree5_before, disagree5_after: as k_mate_overlap indexes them");

static int overlap_check_params(rc_ctx *ctx, const char *who, int32_t min_overlap, int32_t max_mismatch_pct)
{
    if (min_overlap < 1 || min_overlap > RC_OV_MAX_LEN) {
        rc_set_error(ctx, "%s: min_overlap must be 1..%d (got %d)", who, RC_OV_MAX_LEN, min_overlap);
        return RC_ERR_ARG;
    }
    if (max_mismatch_pct < 0 || max_mismatch_pct > 50) {
        rc_set_error(ctx, "%s: max_mismatch_pct must be 0..50 (got %d)", who, max_mismatch_pct);
        return RC_ERR_ARG;
    }
    return RC_OK;
}

extern "C" {

int rc_overlap_stage(rc_ctx *ctx, const rc_device_batch *b, const uint8_t *snap, rc_overlap_staged *st)
{
    st->staged = false;
    rc_ctx *home = rc_home(ctx);
    // (snap == nullptr: no session was open when the batch's bases arrived -- it is in none)
    if (!home->ovl_open || !snap || b->mode == 0 || b->n_reads < 2) return RC_OK;
    if (const int rc = rc_dbuf_reserve(ctx, &st->buf, sizeof(rc_mate_overlap))) return rc;
    RC_CHECK_HIP(ctx, hipMemsetAsync(st->buf.p, 0, sizeof(rc_mate_overlap), ctx->stream));
    st->gen = home->ovl_gen;
    if (const int rc = rc_launch_mate_overlap(ctx, snap, b->d_seq, (size_t)b->nbytes, b->d_off, b->n_reads, b->max_read_len, b->mode, home->ovl_min,
                                              home->ovl_pct, st->buf.p))
        return rc;
    st->staged = true;
    return RC_OK;
}

int rc_overlap_commit(rc_ctx *ctx, rc_overlap_staged *st)
{
    if (!st->staged) return RC_OK;
    st->staged = false;
    rc_ctx *home = rc_home(ctx);
    std::lock_guard<std::mutex> lk(home->obs_mutex);
    if (!home->ovl_open || home->ovl_gen != st->gen) return RC_OK;  // (staged for a session that has ended)
    if (const int rc = rc_launch_trust_add(ctx, st->buf.p, home->ovl_acc, (uint32_t)RC_OVL_WORDS)) return rc;
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

int rc_mate_overlap_device(rc_ctx *ctx, const uint8_t *d_before, const uint8_t *d_after, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                           int32_t max_read_len, int32_t mode, int32_t min_overlap, int32_t max_mismatch_pct, rc_mate_overlap *d_counts)
{
    if (!ctx) return RC_ERR_ARG;
    if (mode < 1 || mode > 2) {
        rc_set_error(ctx, "mate_overlap_device: mode must be 1 or 2, single-end reads have no pairs (got %d)", mode);
        return RC_ERR_ARG;
    }
    if (n_reads & 1u) {
        rc_set_error(ctx, "mate_overlap_device: pairs need an even number of reads (got %u)", n_reads);
        return RC_ERR_ARG;
    }
    if (const int rc = overlap_check_params(ctx, "mate_overlap_device", min_overlap, max_mismatch_pct)) return rc;
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "mate_overlap_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (n_reads && (!d_before || !d_after || !d_off || !d_counts)) {
        rc_set_error(ctx, "mate_overlap_device: null pointer");
        return RC_ERR_ARG;
    }
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_mate_overlap(ctx, d_before, d_after, (size_t)nbytes, d_off, n_reads, max_read_len, mode, min_overlap, max_mismatch_pct, d_counts);
}

int rc_mate_overlap_begin(rc_ctx *ctx, int32_t min_overlap, int32_t max_mismatch_pct)
{
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = overlap_check_params(ctx, "mate_overlap_begin", min_overlap, max_mismatch_pct)) return rc;
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    if (ctx->ovl_open) {
        rc_set_error(ctx, "mate_overlap_begin: a session is open already (rc_mate_overlap_end it first)");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    RC_CHECK_HIP(ctx, hipMalloc(&ctx->ovl_acc, sizeof(rc_mate_overlap)));
    if (hipMemset(ctx->ovl_acc, 0, sizeof(rc_mate_overlap)) != hipSuccess) {
        (void)hipFree(ctx->ovl_acc);
        ctx->ovl_acc = nullptr;
        rc_set_error(ctx, "mate_overlap_begin: could not clear the counts");
        return RC_ERR_HIP;
    }
    ctx->ovl_min = min_overlap;
    ctx->ovl_pct = max_mismatch_pct;
    ++ctx->ovl_gen;
    ctx->ovl_open = true;
    return RC_OK;
}

int rc_mate_overlap_get(rc_ctx *ctx, rc_mate_overlap *out)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->ovl_open) {
        rc_set_error(ctx, "mate_overlap_get: call rc_mate_overlap_begin first");
        return RC_ERR_STATE;
    }
    if (!out) {
        rc_set_error(ctx, "mate_overlap_get: out must not be NULL");
        return RC_ERR_ARG;
    }
    if (const int rc = rc_drain(ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    RC_CHECK_HIP(ctx, hipMemcpy(out, ctx->ovl_acc, sizeof *out, hipMemcpyDeviceToHost));
    out->min_overlap = (uint64_t)ctx->ovl_min;
    out->max_mismatch_pct = (uint64_t)ctx->ovl_pct;
    return RC_OK;
}

int rc_mate_overlap_end(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->ovl_open) {
        rc_set_error(ctx, "mate_overlap_end: no session is open");
        return RC_ERR_STATE;
    }
    const int rc = rc_drain(ctx);  // (a lane's kernel may still write its slot's counts and read its copy of the arena)
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    if (ctx->ovl_acc) (void)hipFree(ctx->ovl_acc);
    ctx->ovl_acc = nullptr;
    ctx->ovl_open = false;
    if (!ctx->rep_acc) {  // (the copies of the arena: the correction report's while it is armed)
        rc_report_release(ctx);
        for (rc_ctx *ln : ctx->lane)
            if (ln) rc_report_release(ln);
    }
    rc_observed_drop_all(ctx, RC_OBS_OVERLAP, true);  // (the staged counts of ctx, its lanes and their slots)
    return rc;
}

}  // extern "C"
