// rc_api_report.hip -- C ABI, the correction report (include/rcorrector_amd.h: rc_change_report; kernel in rc_report.hip):
// arming, reading and releasing it, and the three steps the correction entry points take for it.
//
// Where the counting goes: a batch's arena is copied before its first correction kernel (rc_report_snapshot, on the stream
// of the context the batch runs in) and compared behind the last one (rc_report_count), both in stream order with the
// batch's own kernels -- so a slot's arena, qualities and offsets are done with before the event its wait waits for.  The
// byte entry points have no second submission and count straight into the report.  A packed or resident batch may come
// back with RC_STATUS_NOSPACE and be submitted again: its counts go to a staging block of the slot and reach the report when
// the wait accepts the batch (rc_report_commit) -- once, however often it was submitted.  The three steps are called from
// rc_correct_observed and rc_batch_completed (rc_api_observe.hip), which say where they sit for every entry point.  Slot
// lanes are contexts on streams of their own: they add to the report of the context they serve with device-scope atomics.
// The two paths differ in one respect: a byte batch is in the report once rc_submit has queued its kernels -- if a later step
// of that submit fails, or the caller never waits, it has been counted all the same -- while a staged batch counts only when
// its wait returns success.  Staged counts belong to the report that was armed when the batch was submitted:
// rc_change_report_end drops what the slots still hold, so nothing of an ended report reaches the next one.
#include "rc_api_internal.h"

extern "C" {

int rc_report_snapshot(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, bool pairs, const uint8_t **snap_out)
{
    *snap_out = nullptr;
    const rc_ctx *home = rc_home(ctx);
    // (one copy, whichever of the three wants it, or all; the overlap session wants none of a batch without pairs)
    if ((!home->rep_acc && !(home->ovl_open && pairs) && !home->recur_open) || !nbytes) return RC_OK;
    // at the arena's alignment modulo 16: the kernel reads both in aligned 16-byte pieces (up to 15 bytes on either side)
    const size_t lead = (size_t)((uintptr_t)d_seq & 15u);
    if (const int rc = rc_dbuf_reserve(ctx, &ctx->rep_snap, nbytes + 64)) return rc;
    uint8_t *snap = (uint8_t *)ctx->rep_snap.p + lead;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(snap, d_seq, nbytes, hipMemcpyDeviceToDevice, ctx->stream));
    *snap_out = snap;
    return RC_OK;
}

int rc_report_count(rc_ctx *ctx, const rc_device_batch *b, uint32_t qual_split, uint32_t qual_base2, int qual_bits, const uint8_t *snap,
                    rc_batch_observed *stage)
{
    if (stage) stage->rep_staged = false;
    rc_ctx *home = rc_home(ctx);
    if (!snap || !home->rep_acc || !b->n_reads) return RC_OK;
    unsigned long long *out = home->rep_acc;
    if (stage) {
        if (const int rc = rc_dbuf_reserve(ctx, &stage->rep, RC_REPORT_WORDS * 8)) return rc;
        RC_CHECK_HIP(ctx, hipMemsetAsync(stage->rep.p, 0, RC_REPORT_WORDS * 8, ctx->stream));
        out = (unsigned long long *)stage->rep.p;
    }
    rc_device_batch_args a = rc_device_batch_args();
    a.mode = b->mode;
    a.n = b->n_reads;
    a.seq = b->d_seq;
    a.nbytes = (size_t)b->nbytes;
    a.qual = b->d_qual;
    a.qual_bits = qual_bits >= 0 ? qual_bits : (ctx->qual_bits ? 1 : 0);
    a.qual_split = qual_split;
    a.qual_base2 = qual_base2;
    a.off = b->d_off;
    a.ret = b->d_ret;
    if (const int rc = rc_launch_change_report(ctx, a, snap, out)) return rc;
    if (stage) stage->rep_staged = true;
    return RC_OK;
}

int rc_report_commit(rc_ctx *ctx, const rc_dbuf *staged)
{
    rc_ctx *home = rc_home(ctx);
    if (!home->rep_acc || !staged->p) return RC_OK;
    return rc_launch_report_commit(ctx, (const unsigned long long *)staged->p, home->rep_acc);
}

void rc_report_release(rc_ctx *ctx)
{
    if (ctx->rep_acc) (void)hipFree(ctx->rep_acc);
    ctx->rep_acc = nullptr;
    if (ctx->rep_snap.p) (void)hipFree(ctx->rep_snap.p);
    ctx->rep_snap = rc_dbuf();
}

int rc_change_report_begin(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    if (ctx->rep_acc) {
        rc_set_error(ctx, "change_report_begin: the report is armed already (rc_change_report_end it first)");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    void *p = nullptr;
    RC_CHECK_HIP(ctx, hipMalloc(&p, RC_REPORT_WORDS * 8));
    if (hipMemsetAsync(p, 0, RC_REPORT_WORDS * 8, ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void)hipFree(p);
        rc_set_error(ctx, "change_report_begin: could not clear the accumulator");
        return RC_ERR_HIP;
    }
    ctx->rep_acc = (unsigned long long *)p;
    return RC_OK;
}

int rc_change_report_get(rc_ctx *ctx, rc_change_report *out)
{
    if (!ctx || !out) return RC_ERR_ARG;
    if (!ctx->rep_acc) {
        rc_set_error(ctx, "change_report_get: call rc_change_report_begin first");
        return RC_ERR_STATE;
    }
    static_assert(sizeof(rc_change_report) == RC_REPORT_WORDS * 8, "the accumulator is an rc_change_report");
    if (const int rc = rc_drain(ctx)) return rc;  // (the report kernels of ctx and its lanes have run)
    RC_CHECK_HIP(ctx, hipMemcpy(out, ctx->rep_acc, sizeof *out, hipMemcpyDeviceToHost));
    return RC_OK;
}

int rc_change_report_end(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->rep_acc) {
        rc_set_error(ctx, "change_report_end: the report is not armed");
        return RC_ERR_STATE;
    }
    const int rc = rc_drain(ctx);  // (a lane may still be adding to the accumulator)
    rc_report_release(ctx);
    for (rc_ctx *ln : ctx->lane)
        if (ln) rc_report_release(ln);
    // a packed / resident batch still in flight was counted for this report: its staged counts go with it
    rc_observed_drop_all(ctx, RC_OBS_REPORT, false);
    return rc;
}

}  // extern "C"
