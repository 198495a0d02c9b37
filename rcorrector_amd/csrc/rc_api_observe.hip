// rc_api_observe.hip -- where the batch observers meet the correction entry points: the correction report (rc_api_report.hip),
// the duplicate census (rc_api_dups.hip), the trust profile (rc_api_trust.hip), the mate-overlap report (rc_api_overlap.hip), the
// recurrence census (rc_api_recur.hip) and the recount session that follows corrected batches (rc_api_table.hip: rc_recount_follow).
//
// Every batch entry point hands its batch to rc_correct_observed once the bases lie in HBM, and calls rc_batch_completed where
// the batch is complete and accepted.  Between the two, what the observers took lies in an rc_batch_observed of the slot (or of
// the context, for the entry points that have no slot).  The entry points differ only in what they pass:
//   rc_correct_device                        report direct; completed before it returns, no recount take
//   rc_correct_batch_traced                  report direct; completed behind its final stream synchronise
//   rc_submit / rc_wait                      report direct, at submit; completed in the wait, before the results are copied back
//   rc_submit_packed / rc_submit_resident    report staged; completed in the wait once the fix list fits -- a batch that comes
//                                            back with RC_STATUS_NOSPACE is submitted again and counts then, once
// (rc_correct_read takes the report's snapshot and direct count itself: one read is not a batch of the run.)
// A new observer: its state for one batch into rc_batch_observed (and a bit of RC_OBS_*), its looks at the arena into
// rc_correct_observed, its commit into rc_batch_completed.
#include "rc_api_internal.h"

void rc_batch_observed::drop(int parts, bool free_bufs)
{
    auto release = [free_bufs](rc_dbuf &b) {
        if (!free_bufs) return;
        if (b.p) (void)hipFree(b.p);
        b = rc_dbuf();
    };
    if (parts & RC_OBS_DUPS) {
        dup_units = 0;
        release(dup_keys);
    }
    if (parts & RC_OBS_TRUST) {
        trust.staged = false;
        release(trust.buf);
    }
    if (parts & RC_OBS_OVERLAP) {
        ovl.staged = false;
        release(ovl.buf);
    }
    if (parts & RC_OBS_REPORT) {
        rep_staged = false;
        release(rep);
    }
    if (parts & RC_OBS_RECUR) {
        recur_staged = false;
        recur_n = recur_changes = recur_contexted = 0;
        release(recur_keys);
        release(recur_counts);
    }
}

extern "C" {

void rc_observed_drop_all(rc_ctx *ctx, int parts, bool free_bufs)
{
    auto one = [&](rc_ctx *c) {
        if (!c) return;
        c->obs.drop(parts, free_bufs);
        if (c->slots)
            for (int s = 0; s < RC_MAX_SLOTS; ++s) c->slots[s].obs.drop(parts, free_bufs);
    };
    one(ctx);
    for (rc_ctx *ln : ctx->lane) one(ln);
}

int rc_correct_observed(rc_ctx *ctx, const rc_device_batch *b, uint32_t qual_split, uint32_t qual_base2, int qual_bits, rc_batch_observed *o,
                        bool stage_report)
{
    if (!ctx || !b) return RC_ERR_ARG;
    o->reset();
    if (b->n_reads == 0) return RC_OK;
    int rc;
    if ((rc = rc_correct_check(ctx, b))) return rc;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    // the arena as it arrived ...
    const uint8_t *snap;
    if ((rc = rc_report_snapshot(ctx, b->d_seq, (size_t)b->nbytes, b->mode != 0, &snap))) return rc;
    if ((rc = rc_dups_stage(ctx, b, 0, o))) return rc;
    if ((rc = rc_trust_stage(ctx, b, 0, &o->trust))) return rc;
    if ((rc = rc_correct_device_impl(ctx, b, qual_split, qual_base2, qual_bits))) return rc;
    // ... and as corrected, behind the last correction kernel
    if ((rc = rc_dups_stage(ctx, b, 1, o))) return rc;
    if ((rc = rc_trust_stage(ctx, b, 1, &o->trust))) return rc;
    if ((rc = rc_overlap_stage(ctx, b, snap, &o->ovl))) return rc;
    if ((rc = rc_recur_stage(ctx, b, snap, o))) return rc;
    return rc_report_count(ctx, b, qual_split, qual_base2, qual_bits, snap, stage_report ? o : nullptr);
}

int rc_batch_completed(rc_ctx *ctx, rc_batch_observed *o, const void *d_seq, size_t nbytes)
{
    int rc;
    if (d_seq && (rc = rc_recount_take(ctx, d_seq, nbytes))) return rc;
    if ((rc = rc_dups_commit(ctx, o))) return rc;
    if ((rc = rc_trust_commit(ctx, &o->trust))) return rc;
    if ((rc = rc_overlap_commit(ctx, &o->ovl))) return rc;
    if ((rc = rc_recur_commit(ctx, o))) return rc;
    if (!o->rep_staged) return RC_OK;
    o->rep_staged = false;
    return rc_report_commit(ctx, &o->rep);
}

}  // extern "C"
