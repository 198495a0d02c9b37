// rc_api_internal.h -- what the translation units of the C ABI (rc_api*.hip) share: the context as the ABI layer sees it,
// the slots of the asynchronous transports (rc_api_slots.hip), and the helpers that cross the units.
#pragma once
#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <chrono>
#include <new>
#include <unistd.h>
#include <thread>
#include <vector>

#include "../../include/rcorrector_amd.h"
#include "rc_internal.h"
#include "rc_jfdump.h"

struct rc_ctx_full : rc_ctx {
    rc_dump_cache dump;
};

// pinned host buffer, grow-only
struct rc_hbuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// what a slot holds (rc_api_slots.hip): nothing -- it is free -- or a batch of one of the three transports, whose wait alone takes it
enum rc_slot_kind { RC_SLOT_NONE, RC_SLOT_BYTES, RC_SLOT_PACKED, RC_SLOT_RESIDENT };

// where a packed / resident batch's outputs go: the arrays of the caller's descriptor (valid until its wait) and its n_fix
struct rc_slot_out {
    int32_t *ret = nullptr, *l = nullptr, *m = nullptr, *h = nullptr;
    uint32_t *fix_pos = nullptr;
    uint8_t *fix_chr = nullptr;
    size_t *n_fix = nullptr;
};

// 16 bytes per read that a batch in flight computes behind its last correction kernel for a one-shot registration: the
// caller's array (nullptr: none asked for), whether it is page-locked, the values in HBM, and their staging where it is not
struct rc_slot_payload {
    void *out = nullptr;
    bool pinned = false;
    rc_dbuf d;
    rc_hbuf p;
};

// one batch in flight on the asynchronous slot transports
struct rc_slot {
    rc_slot_kind kind = RC_SLOT_NONE;
    size_t total_reads = 0;          // reads of the batch over both arenas (0: an empty batch, nothing was queued)
    size_t arena_bytes = 0;          // bytes of the batch's arena in d_seq (what rc_recount_follow takes when the batch completes)
    bool res_pinned = false;         // the caller's result arrays are page-locked: DMA straight to them, else through p_res
    rc_hbuf p_res;
    rc_dbuf d_seq, d_qual, d_off, d_res;
    hipEvent_t e_h2d = nullptr, e_k = nullptr, e_done = nullptr;
    // the byte transport (rc_submit): the caller's descriptor (its buffers stay valid until rc_wait), the two arenas' sizes,
    // and pinned staging for the offsets and for arenas that are pageable
    rc_batch b;
    size_t bytes1 = 0, bytes2 = 0;
    bool seq_pinned = false;
    rc_hbuf p_seq, p_qual, p_off;
    // the packed and the resident transport: the outputs, the packed arena / exceptions / fix count in HBM (resident: the
    // count only, its arena is copied from the counter's kept arenas), pinned staging for descriptor arrays that are not
    // page-locked, and the fix count's landing place
    rc_slot_out out;
    rc_dbuf d_packed, d_exc, d_fix;
    rc_hbuf p_in, p_fix, p_nfix;
    // the per-read payloads of the batch in flight, 16 bytes per read each, by rc_payload_kind
    rc_slot_payload payload[RC_PAY_COUNT];
    // what the batch observers staged for the batch in flight, until its wait accepts it (a packed / resident batch that did
    // not fit its fix list comes again, and only then counts)
    rc_batch_observed obs;
    uint32_t fix_room = 0;
    bool fix_pinned = false;
};

// one rc_device_batch over a result block d_res = ret | l | m | h of `total` reads each
static inline rc_device_batch rc_device_batch_over(int mode, size_t total, size_t nbytes, int max_len, uint8_t *d_seq, const uint8_t *d_qual,
                                                   const uint32_t *d_off, int32_t *d_res)
{
    rc_device_batch db;
    db.mode = mode;
    db.n_reads = (uint32_t)total;
    db.nbytes = nbytes;
    db.max_read_len = max_len;
    db.d_seq = d_seq;
    db.d_qual = d_qual;
    db.d_off = d_off;
    db.d_ret = d_res;
    db.d_l = d_res + total;
    db.d_m = d_res + 2 * total;
    db.d_h = d_res + 3 * total;
    return db;
}

// the offsets of a host batch's device arena -- arena 1, then (mode 1) arena 2 behind arena 1's bytes1 bytes -- into off[total + 1];
// returns the longest read, in bases
static inline int rc_concat_offsets(const rc_batch *b, size_t bytes1, uint32_t *off)
{
    const size_t n1 = b->n;
    int max_len = 0;
    memcpy(off, b->off, (n1 + 1) * 4);
    for (size_t i = 0; i < n1; ++i) max_len = std::max(max_len, (int)(b->off[i + 1] - b->off[i]) - 1);
    if (b->mode == 1) {
        for (size_t i = 0; i <= n1; ++i) off[n1 + i] = (uint32_t)bytes1 + b->off2[i];
        for (size_t i = 0; i < n1; ++i) max_len = std::max(max_len, (int)(b->off2[i + 1] - b->off2[i]) - 1);
    }
    return max_len;
}

extern "C" {  // (defined inside the units' extern "C" blocks)
// rc_api_batch.hip
// check: what every correction entry point refuses of a batch descriptor with reads in it (status and error text).  impl: the
// correction kernels over a batch that passed it, on ctx's stream with ctx's device current -- only rc_correct_observed calls
// the two.  qual_split / qual_base2 (quality-bit mode only): arena bytes from qual_split on have their bits at byte qual_base2
// of d_qual; qual_bits: -1 = as rc_set_quality_bits says, 0 / 1 = this batch's quality arena holds bytes / bits (the packed boundary)
int rc_correct_check(rc_ctx *ctx, const rc_device_batch *b);
int rc_correct_device_impl(rc_ctx *ctx, const rc_device_batch *b, uint32_t qual_split, uint32_t qual_base2, int qual_bits);
// rc_api_observe.hip -- the one place the batch observers (correction report, duplicate census, trust profile, mate-overlap
// report, recount follow) are hooked in.  ctx is the context the batch runs in (a context or one of its slot lanes).
// rc_correct_observed: what every batch entry point does with its batch once the bases lie in b->d_seq -- rc_correct_check
// (a refused batch reaches no observer; an empty one is RC_OK with nothing staged), then on ctx's stream the observers' look at
// the arena as it is, rc_correct_device_impl, and their look at it as corrected, staged into o.  stage_report: the report's
// counts wait in o too (a batch whose wait may refuse it), else they go straight into the report.
// rc_batch_completed: the batch has completed and is accepted -- its corrected arena to the recount session (d_seq == nullptr:
// not for this entry point), then what o holds into the census, the profile and the report, o empty afterwards; once per batch.
int rc_correct_observed(rc_ctx *ctx, const rc_device_batch *b, uint32_t qual_split, uint32_t qual_base2, int qual_bits, rc_batch_observed *o,
                        bool stage_report);
int rc_batch_completed(rc_ctx *ctx, rc_batch_observed *o, const void *d_seq, size_t nbytes);
// o->drop(parts, free_bufs) for the rc_batch_observed of ctx, of its slots, and of its lanes and their slots
void rc_observed_drop_all(rc_ctx *ctx, int parts, bool free_bufs);
// rc_api_slots.hip
int rc_hbuf_reserve(rc_ctx *ctx, rc_hbuf *h, size_t bytes);
bool rc_is_pinned(const void *p, size_t bytes);
int rc_slots_init(rc_ctx *ctx);
// rc_api.hip
// the context slot `slot` runs in: ctx itself (slot 0, a lane, or RC_SLOT_LANES=0), else its lane -- created if `create`, and
// brought up to date with ctx's table / parameters / kept arenas if `refresh` (submits); nullptr + error text on failure
rc_ctx *rc_slot_lane(rc_ctx *ctx, int slot, bool create, bool refresh);
// the lane's error text and summary counters seen through the parent
void rc_lane_error(rc_ctx *ctx, const rc_ctx *lane);
// The observers' own steps, called from rc_correct_observed / rc_batch_completed (and, the report's first two, from
// rc_correct_read, whose one read is no batch of the run).  All do nothing while their observer is not armed; the accumulator
// is that of rc_home(ctx), the context the batch was submitted to.
// rc_api_table.hip
// rc_recount_follow: the corrected arena in d_seq appended to the open session, on ctx's own stream; nothing without a session
int rc_recount_take(rc_ctx *ctx, const void *d_seq, size_t nbytes);
// rc_api_report.hip -- snapshot: the arena as it is, copied on ctx's stream, where the report is armed, a recurrence census is
// open, or a mate-overlap session is open and the batch has pairs (one copy for all; a single-end batch is not copied for the
// overlap session alone); *snap = where (nullptr: none was taken).
// count: the batch against that snapshot, straight into the report (stage == nullptr) or into stage->rep (zeroed first;
// stage->rep_staged = something was launched).  commit: a staged block into the report.
int rc_report_snapshot(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, bool pairs, const uint8_t **snap);
int rc_report_count(rc_ctx *ctx, const rc_device_batch *b, uint32_t qual_split, uint32_t qual_base2, int qual_bits, const uint8_t *snap,
                    rc_batch_observed *stage);
int rc_report_commit(rc_ctx *ctx, const rc_dbuf *staged);
void rc_report_release(rc_ctx *ctx);
// rc_api_dups.hip -- stage: the keys of the batch's arena as it is now, on ctx's stream, into o->dup_keys (version 0 reserves
// them for both versions and sets o->dup_units / dup_gen).  commit: appended to the census, complete on return; o->dup_units = 0.
int rc_dups_stage(rc_ctx *ctx, const rc_device_batch *b, int version, rc_batch_observed *o);
int rc_dups_commit(rc_ctx *ctx, rc_batch_observed *o);
// rc_api_trust.hip -- stage: version 0 zeroes st's two rc_trust_counts and counts the arena as it is into the first, version 1
// into the second, on ctx's stream.  commit: the pair added to the profile, complete on return.
int rc_trust_stage(rc_ctx *ctx, const rc_device_batch *b, int version, rc_trust_staged *st);
int rc_trust_commit(rc_ctx *ctx, rc_trust_staged *st);
// rc_api_overlap.hip -- stage: behind the last correction kernel, st's rc_mate_overlap zeroed and the batch's pairs counted
// into it, snap (rc_report_snapshot's) against the arena as corrected, on ctx's stream; a single-end batch stages nothing.
// commit: added to the session, complete on return.
int rc_overlap_stage(rc_ctx *ctx, const rc_device_batch *b, const uint8_t *snap, rc_overlap_staged *st);
int rc_overlap_commit(rc_ctx *ctx, rc_overlap_staged *st);
// rc_api_recur.hip -- stage: behind the last correction kernel, the site keys of the batch's contexted changes, snap
// (rc_report_snapshot's) against the arena as corrected, into o->recur_keys; WAITS for ctx's stream to learn their number (and
// launches again into a larger buffer where they did not fit).  commit: appended to the census, complete on return.
int rc_recur_stage(rc_ctx *ctx, const rc_device_batch *b, const uint8_t *snap, rc_batch_observed *o);
int rc_recur_commit(rc_ctx *ctx, rc_batch_observed *o);
void rc_recur_release(rc_ctx *ctx);
}
