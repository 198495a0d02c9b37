// rc_api_slots.hip -- C ABI, the three asynchronous slot transports (include/rcorrector_amd.h): rc_submit / rc_wait (byte
// arenas), rc_submit_packed / rc_wait_packed (2-bit bases / quality bits / offsets down, ret / l / m / h + a fix list up;
// device side in rc_transport.hip) and rc_submit_resident / rc_wait_resident (reads the counter kept in HBM: offsets and
// quality bits only).  The steps the transports have in common exist once, in front of the entry points.
#include "rc_api_internal.h"

// The reference overlaps the I/O of batch N+1 with the correction of batch N by handing batches to
// worker threads (main.cpp:479-516).  Here one context keeps up to RC_MAX_SLOTS batches in flight on
// three streams: H2D(N+1) || kernels(N) || D2H(N-1).  Scratch memory of the kernels is shared --
// they serialise on the compute stream -- only the arenas and result arrays exist per slot.

// ---- the shared steps --------------------------------------------------------------------------
// Slot lanes (rc_internal.h): a slot above 0 may run in a context of its own, as that context's slot 0.  entry(ctx, slot)
// is the entry point's body; a submit creates the lane and brings it up to date, a wait goes where the batch went.
template <class Entry>
static int in_slot_lane(rc_ctx *c, int slot, bool submit, Entry entry)
{
    if (!c || slot < 0 || slot >= RC_MAX_SLOTS) return RC_ERR_ARG;
    // a submit takes the slot's registrations (rc_weak_profile_into, rc_read_depth_into, rc_read_screen_into) with it, whatever
    // becomes of the submit
    rc_ctx::rc_payload_reg reg[RC_PAY_COUNT];
    if (submit)
        for (int kind = 0; kind < RC_PAY_COUNT; ++kind) std::swap(reg[kind], c->payload_reg[kind][slot]);
    rc_ctx *ln = rc_slot_lane(c, slot, submit, submit);
    if (!ln) return RC_ERR_HIP;
    if (submit) std::copy(reg, reg + RC_PAY_COUNT, ln->payload_cur);
    const int rc = entry(static_cast<rc_ctx_full *>(ln), ln == c ? slot : 0);
    // (a submit that returned in front of slot_download: nothing stays behind)
    if (submit) std::fill(ln->payload_cur, ln->payload_cur + RC_PAY_COUNT, rc_ctx::rc_payload_reg());
    if (rc && ln != c) rc_lane_error(c, ln);
    return rc;
}

// a submit's slot: the device current, the slots there, this one free (`wait_hint`: what `name`'s message tells the caller to do)
static int slot_acquire(rc_ctx_full *ctx, int slot, const char *name, const char *wait_hint, rc_slot **out)
{
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (const int rc = rc_slots_init(ctx)) return rc;
    rc_slot &sl = ctx->slots[slot];
    if (sl.kind != RC_SLOT_NONE) {
        rc_set_error(ctx, "%s: slot %d still holds a batch (%s first)", name, slot, wait_hint);
        return RC_ERR_STATE;
    }
    for (rc_slot_payload &pl : sl.payload) pl.out = nullptr;  // (slot_download sets them for a batch that has the registration)
    sl.obs.reset();         // (rc_correct_observed stages into it what the armed observers take of the batch)
    *out = &sl;
    return RC_OK;
}

// a wait's slot: the batch of `kind` it holds (`what`: the kind in words), the slot free again; nullptr + error text without one
static rc_slot *slot_take(rc_ctx_full *ctx, int slot, rc_slot_kind kind, const char *name, const char *what)
{
    if (!ctx->slots || ctx->slots[slot].kind != kind) {
        rc_set_error(ctx, "%s: slot %d holds no %sbatch", name, slot, what);
        return nullptr;
    }
    ctx->slots[slot].kind = RC_SLOT_NONE;
    return &ctx->slots[slot];
}

// The offsets of a packed / resident batch, in the entry points' order of refusal: they span the arena (`spans`: what else the
// transport asks of them; ends_fmt takes off[0], total, off[total], nbytes), a table is loaded, and every read ends with its
// NUL -- strictly ascending offsets (the terminator / exception kernels write seq[off[i+1]-1] and seq[exc_pos[i]] unchecked).
static int slot_check_offsets(rc_ctx_full *ctx, const char *name, const uint32_t *off, size_t total, size_t nbytes, bool spans, const char *ends_fmt,
                              int *max_len)
{
    if (off[0] != 0 || off[total] != nbytes || !spans) {
        rc_set_error(ctx, ends_fmt, off[0], total, off[total], nbytes);
        return RC_ERR_ARG;
    }
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "correct: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    *max_len = 0;
    for (size_t i = 0; i < total; ++i) {
        if (off[i + 1] <= off[i]) {
            rc_set_error(ctx, "%s: off[%zu] = %u, off[%zu] = %u: offsets must ascend (a read is its bases and a NUL)", name, i, off[i], i + 1, off[i + 1]);
            return RC_ERR_ARG;
        }
        *max_len = std::max(*max_len, (int)(off[i + 1] - off[i]) - 1);
    }
    return RC_OK;
}

// From the first copy on, copies are in flight from the caller's buffers (or the slot's staging): an error must not
// return before they have drained, or the caller could free / the next submit could overwrite memory the
// DMA engines still read.  Armed after a submit's last reservation, disarmed when the batch is in the slot.
namespace {
struct drain_on_error {
    rc_ctx *c;
    bool armed = true;
    ~drain_on_error()
    {
        if (!armed) return;
        (void)hipStreamSynchronize(c->s_h2d);
        (void)hipStreamSynchronize(c->stream);
        (void)hipStreamSynchronize(c->s_d2h);
    }
};
}  // namespace

// where a packed / resident batch's outputs land: straight in the caller's arrays where those are page-locked, else in staging
// of the slot's that the wait copies from
static int slot_outputs(rc_ctx_full *ctx, rc_slot &sl, const rc_slot_out &out, size_t total, uint32_t cap)
{
    sl.out = out;
    sl.res_pinned = rc_is_pinned(out.ret, total * 4) && rc_is_pinned(out.l, total * 4) && rc_is_pinned(out.m, total * 4) && rc_is_pinned(out.h, total * 4);
    sl.fix_pinned = !cap || (rc_is_pinned(out.fix_pos, (size_t)cap * 4) && rc_is_pinned(out.fix_chr, cap));
    sl.fix_room = cap;
    int rc;
    if (!sl.res_pinned && (rc = rc_hbuf_reserve(ctx, &sl.p_res, total * 16))) return rc;
    if (!sl.fix_pinned && (rc = rc_hbuf_reserve(ctx, &sl.p_fix, (size_t)cap * 5 + 64))) return rc;
    return RC_OK;
}

// The fix list is written by the kernel straight into page-locked host memory (the caller's arrays, or the slot's
// staging where those are pageable): a few bytes per read, consecutive entries from consecutive lanes.  A copy after
// the kernels would have to wait for the count first -- a second round trip per batch on a stream of its own, which
// on this runtime shares a hardware queue with one of the other four and stalls behind it.
static int slot_fix_list_target(rc_ctx_full *ctx, const rc_slot &sl, uint32_t **d_fix_pos, uint8_t **d_fix_chr)
{
    void *dp = nullptr, *dc = nullptr;
    if (sl.fix_room) {
        RC_CHECK_HIP(ctx, hipHostGetDevicePointer(&dp, sl.fix_pinned ? (void *)sl.out.fix_pos : sl.p_fix.p, 0));
        RC_CHECK_HIP(ctx, hipHostGetDevicePointer(&dc, sl.fix_pinned ? (void *)sl.out.fix_chr : (void *)((char *)sl.p_fix.p + (size_t)sl.fix_room * 4), 0));
    }
    *d_fix_pos = (uint32_t *)dp;
    *d_fix_chr = (uint8_t *)dc;
    return RC_OK;
}

// A per-read payload (rc_api_internal.h: rc_slot_payload), the steps of its way.  reserve: the registration's array into
// the slot, with room for the values in HBM and, where the array is not page-locked, in the slot's staging; nothing for out ==
// nullptr.  download: the 16 bytes per read on the download stream, into the array or the staging.  back: a wait that succeeds
// hands over what went to the staging.
static int payload_reserve(rc_ctx_full *ctx, rc_slot_payload &pl, void *out, size_t total)
{
    pl.out = out;
    if (!out) return RC_OK;
    if (const int rc = rc_dbuf_reserve(ctx, &pl.d, total * 16)) return rc;
    pl.pinned = rc_is_pinned(out, total * 16);
    return pl.pinned ? (int)RC_OK : rc_hbuf_reserve(ctx, &pl.p, total * 16);
}

// the kernels of payload `kind` over the slot's corrected arena, on ctx's compute stream, where the batch has the registration
// -- the one place that knows the kinds apart
static int payload_launch(rc_ctx_full *ctx, rc_slot &sl, int kind, const rc_ctx::rc_payload_reg &reg)
{
    if (!sl.payload[kind].out) return RC_OK;
    const uint8_t *d_seq = (const uint8_t *)sl.d_seq.p;
    const uint32_t *d_off = (const uint32_t *)sl.d_off.p;
    const uint32_t n = (uint32_t)sl.total_reads;
    void *d_out = sl.payload[kind].d.p;
    switch (kind) {
    case RC_PAY_WEAK: return rc_launch_weak_profile(ctx, d_seq, sl.arena_bytes, d_off, n, reg.min_count, &ctx->weak_planes, d_out);
    case RC_PAY_DEPTH: return rc_launch_read_depth(ctx, d_seq, sl.arena_bytes, d_off, n, d_out);
    default: return rc_launch_read_screen(ctx, reg.screen, d_seq, sl.arena_bytes, d_off, n, reg.min_count, d_out);
    }
}

static int payload_download(rc_ctx_full *ctx, const rc_slot_payload &pl, size_t total)
{
    if (pl.out) RC_CHECK_HIP(ctx, hipMemcpyAsync(pl.pinned ? pl.out : pl.p.p, pl.d.p, total * 16, hipMemcpyDeviceToHost, ctx->s_d2h));
    return RC_OK;
}

static void payload_back(const rc_slot_payload &pl, size_t total)
{
    if (pl.out && !pl.pinned) memcpy(pl.out, pl.p.p, total * 16);
}

// Behind the batch's last kernel: what `first` queues on the download stream (the arena, the fix count), then ret / l / m / h to
// sl.out or the slot's staging.  one_copy: where the caller's four arrays are one block, as the device's are, one copy instead
// of four.  A batch submitted with a payload registration (rc_api_payload.hip: ctx->payload_cur) has that payload's kernels run
// over its corrected arena first, behind its last kernel on its own stream, and the 16 bytes per read come down with the
// results -- weak profile, depth, screen, in rc_payload_kind's order on either stream.
template <class First>
static int slot_download(rc_ctx_full *ctx, rc_slot &sl, bool one_copy, First first)
{
    const size_t total = sl.total_reads;
    const rc_slot_out &o = sl.out;
    const int32_t *d_res = (const int32_t *)sl.d_res.p;
    rc_ctx::rc_payload_reg reg[RC_PAY_COUNT];
    for (int kind = 0; kind < RC_PAY_COUNT; ++kind) std::swap(reg[kind], ctx->payload_cur[kind]);
    for (int kind = 0; kind < RC_PAY_COUNT; ++kind) {
        if (const int rc = payload_reserve(ctx, sl.payload[kind], reg[kind].out, total)) return rc;
        if (const int rc = payload_launch(ctx, sl, kind, reg[kind])) return rc;
    }
    RC_CHECK_HIP(ctx, hipEventRecord(sl.e_k, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamWaitEvent(ctx->s_d2h, sl.e_k, 0));
    if (const int rc = first()) return rc;
    for (const rc_slot_payload &pl : sl.payload)
        if (const int rc = payload_download(ctx, pl, total)) return rc;
    if (!sl.res_pinned) {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.p_res.p, d_res, total * 16, hipMemcpyDeviceToHost, ctx->s_d2h));
    } else if (one_copy && o.l == o.ret + total && o.m == o.l + total && o.h == o.m + total) {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(o.ret, d_res, total * 16, hipMemcpyDeviceToHost, ctx->s_d2h));
    } else {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(o.ret, d_res, total * 4, hipMemcpyDeviceToHost, ctx->s_d2h));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(o.l, d_res + total, total * 4, hipMemcpyDeviceToHost, ctx->s_d2h));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(o.m, d_res + 2 * total, total * 4, hipMemcpyDeviceToHost, ctx->s_d2h));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(o.h, d_res + 3 * total, total * 4, hipMemcpyDeviceToHost, ctx->s_d2h));
    }
    RC_CHECK_HIP(ctx, hipEventRecord(sl.e_done, ctx->s_d2h));
    return RC_OK;
}

// a wait: results that went to the slot's staging, into the caller's arrays
static void slot_results_back(const rc_slot &sl)
{
    const size_t total = sl.total_reads;
    for (const rc_slot_payload &pl : sl.payload) payload_back(pl, total);
    if (sl.res_pinned) return;
    const int32_t *r = (const int32_t *)sl.p_res.p;
    memcpy(sl.out.ret, r, total * 4);
    memcpy(sl.out.l, r + total, total * 4);
    memcpy(sl.out.m, r + 2 * total, total * 4);
    memcpy(sl.out.h, r + 3 * total, total * 4);
}

// the wait of a batch with a fix list, from the moment the slot is free again
static int slot_wait_fix_list(rc_ctx_full *ctx, rc_slot &sl, const char *name)
{
    if (sl.total_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    RC_CHECK_HIP(ctx, hipEventSynchronize(sl.e_done));  // the results and the fix count have landed; the list was written by the kernel
    const uint32_t n_fix = *(const volatile uint32_t *)sl.p_nfix.p, cap = sl.fix_room;
    if (n_fix > cap) {  // (the kernel stopped writing at cap; the results are complete, the list is not)
        *sl.out.n_fix = n_fix;
        rc_set_error(ctx, "%s: %u substitutions, room for %u (fix_cap)", name, n_fix, cap);
        return RC_ERR_NOSPACE;
    }
    // the observers: before the slot can be reused, and only now (a batch that did not fit its fix list comes again and counts then)
    if (const int frc = rc_batch_completed(ctx, &sl.obs, sl.d_seq.p, sl.arena_bytes)) return frc;
    slot_results_back(sl);
    if (!sl.fix_pinned && n_fix) {
        memcpy(sl.out.fix_pos, sl.p_fix.p, (size_t)n_fix * 4);
        memcpy(sl.out.fix_chr, (const uint8_t *)sl.p_fix.p + (size_t)cap * 4, n_fix);
    }
    *sl.out.n_fix = n_fix;
    return RC_OK;
}

// ---- the byte transport --------------------------------------------------------------------------
static int submit_bytes(rc_ctx_full *ctx, const rc_batch *b, int slot)
{
    if (b->mode < 0 || b->mode > 2 || (b->n && (!b->seq || !b->qual || !b->off || !b->ret || !b->l || !b->m || !b->h)) ||
        (b->n && b->mode == 1 && (!b->seq2 || !b->qual2 || !b->off2))) {
        rc_set_error(ctx, "submit: bad batch descriptor");
        return RC_ERR_ARG;
    }
    rc_slot *slp;
    int rc = slot_acquire(ctx, slot, "submit", "rc_wait it", &slp);
    if (rc) return rc;
    rc_slot &sl = *slp;
    sl.b = *b;
    const size_t n1 = b->n;
    sl.total_reads = b->mode == 1 ? 2 * n1 : n1;
    sl.bytes1 = n1 ? b->off[n1] : 0;
    sl.bytes2 = (n1 && b->mode == 1) ? b->off2[n1] : 0;
    if (n1 == 0) {
        sl.kind = RC_SLOT_BYTES;
        return RC_OK;
    }
    const size_t nbytes = sl.bytes1 + sl.bytes2, total = sl.total_reads;
    sl.arena_bytes = nbytes;
    if (nbytes >= (1ull << 32) || total >= (1ull << 32)) {
        rc_set_error(ctx, "submit: batch too large (split it)");
        return RC_ERR_ARG;
    }
    if (b->mode == 2 && (n1 & 1)) {  // (before any copy is queued)
        rc_set_error(ctx, "submit: interleaved mode needs an even number of reads (got %zu)", n1);
        return RC_ERR_ARG;
    }
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "correct: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    // offsets of the device arena and the longest read, into pinned memory
    if ((rc = rc_hbuf_reserve(ctx, &sl.p_off, (total + 1) * 4))) return rc;
    uint32_t *off = (uint32_t *)sl.p_off.p;
    const int max_len = rc_concat_offsets(b, sl.bytes1, off);
    // quality arenas: a byte per base, or (rc_set_quality_bits) a bit per arena byte, arena 2's bits in
    // a region of their own
    const bool qbits = ctx->qual_bits;
    const size_t q1 = qbits ? (sl.bytes1 + 7) / 8 : sl.bytes1, q2 = qbits ? (sl.bytes2 + 7) / 8 : sl.bytes2;
    const size_t qbase2 = qbits ? ((q1 + 15) & ~(size_t)15) : sl.bytes1;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_seq, nbytes + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_qual, qbase2 + q2 + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_off, (total + 1) * 4))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_res, total * 16))) return rc;
    sl.seq_pinned = rc_is_pinned(b->seq, sl.bytes1) && rc_is_pinned(b->qual, q1) &&
                    (b->mode != 1 || (rc_is_pinned(b->seq2, sl.bytes2) && rc_is_pinned(b->qual2, q2)));
    sl.out = rc_slot_out{b->ret, b->l, b->m, b->h};
    sl.res_pinned = rc_is_pinned(b->ret, total * 4) && rc_is_pinned(b->l, total * 4) && rc_is_pinned(b->m, total * 4) && rc_is_pinned(b->h, total * 4);
    const char *h_seq1 = b->seq, *h_qual1 = b->qual, *h_seq2 = b->seq2, *h_qual2 = b->qual2;
    if (!sl.seq_pinned) {  // pageable buffers: through the slot's pinned staging
        if ((rc = rc_hbuf_reserve(ctx, &sl.p_seq, nbytes))) return rc;
        if ((rc = rc_hbuf_reserve(ctx, &sl.p_qual, qbase2 + q2))) return rc;
        memcpy(sl.p_seq.p, b->seq, sl.bytes1);
        memcpy(sl.p_qual.p, b->qual, q1);
        if (b->mode == 1) {
            memcpy((char *)sl.p_seq.p + sl.bytes1, b->seq2, sl.bytes2);
            memcpy((char *)sl.p_qual.p + qbase2, b->qual2, q2);
        }
        h_seq1 = (const char *)sl.p_seq.p;
        h_qual1 = (const char *)sl.p_qual.p;
        h_seq2 = h_seq1 + sl.bytes1;
        h_qual2 = h_qual1 + qbase2;
    }
    if (!sl.res_pinned && (rc = rc_hbuf_reserve(ctx, &sl.p_res, total * 16))) return rc;
    uint8_t *d_seq = (uint8_t *)sl.d_seq.p, *d_qual = (uint8_t *)sl.d_qual.p;
    // one upload stream: bases and qualities on two streams measured 21 GB/s against 26.6 GB/s on one
    // (the link, not a DMA engine, is the bound)
    drain_on_error guard{ctx};
    RC_CHECK_HIP(ctx, hipMemcpyAsync(d_seq, h_seq1, sl.bytes1, hipMemcpyHostToDevice, ctx->s_h2d));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(d_qual, h_qual1, q1, hipMemcpyHostToDevice, ctx->s_h2d));
    if (b->mode == 1) {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(d_seq + sl.bytes1, h_seq2, sl.bytes2, hipMemcpyHostToDevice, ctx->s_h2d));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(d_qual + qbase2, h_qual2, q2, hipMemcpyHostToDevice, ctx->s_h2d));
    }
    RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.d_off.p, off, (total + 1) * 4, hipMemcpyHostToDevice, ctx->s_h2d));
    RC_CHECK_HIP(ctx, hipEventRecord(sl.e_h2d, ctx->s_h2d));
    // kernels
    RC_CHECK_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl.e_h2d, 0));
    const rc_device_batch db = rc_device_batch_over(b->mode, total, nbytes, max_len, d_seq, d_qual, (const uint32_t *)sl.d_off.p, (int32_t *)sl.d_res.p);
    const uint32_t qsplit = qbits && b->mode == 1 ? (uint32_t)sl.bytes1 : 0xFFFFFFFFu;
    // (the correction report: no second submission on this path -- counted here, before the event rc_wait waits for)
    if ((rc = rc_correct_observed(ctx, &db, qsplit, (uint32_t)qbase2, -1, &sl.obs, false))) return rc;
    // the corrected arena, then the results: always to the caller's four arrays one by one
    rc = slot_download(ctx, sl, false, [&]() -> int {
        char *o_seq1 = sl.seq_pinned ? b->seq : (char *)sl.p_seq.p;
        RC_CHECK_HIP(ctx, hipMemcpyAsync(o_seq1, d_seq, sl.bytes1, hipMemcpyDeviceToHost, ctx->s_d2h));
        if (b->mode == 1) {
            char *o_seq2 = sl.seq_pinned ? b->seq2 : (char *)sl.p_seq.p + sl.bytes1;
            RC_CHECK_HIP(ctx, hipMemcpyAsync(o_seq2, d_seq + sl.bytes1, sl.bytes2, hipMemcpyDeviceToHost, ctx->s_d2h));
        }
        return RC_OK;
    });
    if (rc) return rc;
    guard.armed = false;
    sl.kind = RC_SLOT_BYTES;
    return RC_OK;
}

static int wait_bytes(rc_ctx_full *ctx, int slot)
{
    if (ctx->slots && (ctx->slots[slot].kind == RC_SLOT_PACKED || ctx->slots[slot].kind == RC_SLOT_RESIDENT)) {
        rc_set_error(ctx, "wait: slot %d holds a packed batch (rc_wait_packed / rc_wait_resident)", slot);
        return RC_ERR_STATE;
    }
    rc_slot *slp = slot_take(ctx, slot, RC_SLOT_BYTES, "wait", "");
    if (!slp) return RC_ERR_STATE;
    rc_slot &sl = *slp;
    if (sl.total_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    RC_CHECK_HIP(ctx, hipEventSynchronize(sl.e_done));
    if (const int frc = rc_batch_completed(ctx, &sl.obs, sl.d_seq.p, sl.arena_bytes)) return frc;  // (the observers: before the slot can be reused)
    if (!sl.seq_pinned) {
        memcpy(sl.b.seq, sl.p_seq.p, sl.bytes1);
        if (sl.b.mode == 1) memcpy(sl.b.seq2, (char *)sl.p_seq.p + sl.bytes1, sl.bytes2);
    }
    slot_results_back(sl);
    return RC_OK;
}

// ---- the packed transport --------------------------------------------------------------------------
static int submit_packed(rc_ctx_full *ctx, rc_packed_batch *b, int slot)
{
    if (b->mode < 0 || b->mode > 2 || (b->n && (!b->off || !b->bases || !b->ret || !b->l || !b->m || !b->h)) ||
        (b->n_exc && (!b->exc_pos || !b->exc_chr)) || (b->fix_cap && (!b->fix_pos || !b->fix_chr))) {
        rc_set_error(ctx, "submit_packed: bad batch descriptor");
        return RC_ERR_ARG;
    }
    rc_slot *slp;
    int rc = slot_acquire(ctx, slot, "submit_packed", "rc_wait_packed it", &slp);
    if (rc) return rc;
    rc_slot &sl = *slp;
    const size_t total = b->mode == 1 ? 2 * b->n : b->n, nbytes = (size_t)b->nbytes;
    b->n_fix = 0;
    if (total == 0) {
        sl.total_reads = 0;
        sl.kind = RC_SLOT_PACKED;
        return RC_OK;
    }
    if (nbytes >= (1ull << 32) || total >= (1ull << 32) || b->n_exc >= (1ull << 32) || b->fix_cap >= (1ull << 32)) {
        rc_set_error(ctx, "submit_packed: batch too large (split it)");
        return RC_ERR_ARG;
    }
    if (b->mode != 0 && (total & 1)) {
        rc_set_error(ctx, "submit_packed: %s mode needs an even number of reads", b->mode == 1 ? "paired" : "interleaved");
        return RC_ERR_ARG;
    }
    int max_len;
    if ((rc = slot_check_offsets(ctx, "submit_packed", b->off, total, nbytes, true,
                                 "submit_packed: off[0] = %u, off[%zu] = %u do not describe the arena's %zu bytes", &max_len)))
        return rc;
    for (size_t i = 0; i < b->n_exc; ++i)
        if (b->exc_pos[i] >= nbytes) {
            rc_set_error(ctx, "submit_packed: exc_pos[%zu] = %u lies outside the arena's %zu bytes", i, b->exc_pos[i], nbytes);
            return RC_ERR_ARG;
        }
    sl.total_reads = total;
    const size_t n_words = (nbytes + 15) / 16, qb = (nbytes + 7) / 8, n_exc = b->n_exc;
    sl.arena_bytes = nbytes;
    const uint32_t cap = (uint32_t)b->fix_cap;
    // device memory: the packed arena, the byte arena it expands into, qualities, offsets, results, exceptions, fixes
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_packed, n_words * 4 + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_seq, n_words * 16 + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_qual, (b->qual_bits ? qb : nbytes) + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_off, (total + 1) * 4))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_res, total * 16))) return rc;
    const size_t exc_chr_off = ((size_t)n_exc * 4 + 15) & ~(size_t)15;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_exc, exc_chr_off + n_exc + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_fix, 64))) return rc;  // (the count; the list itself goes to host memory)
    if ((rc = rc_hbuf_reserve(ctx, &sl.p_nfix, 64))) return rc;
    // inputs that are not page-locked go through one staging block of the slot
    const bool in_pinned = rc_is_pinned(b->off, (total + 1) * 4) && rc_is_pinned(b->bases, n_words * 4) && (!b->qual_bits || rc_is_pinned(b->qual_bits, qb)) &&
                           (!n_exc || (rc_is_pinned(b->exc_pos, n_exc * 4) && rc_is_pinned(b->exc_chr, n_exc)));
    const uint32_t *h_off = b->off, *h_bases = b->bases, *h_exc_pos = b->exc_pos;
    const uint8_t *h_qb = b->qual_bits, *h_exc_chr = b->exc_chr;
    if (!in_pinned) {
        const size_t o_bases = ((total + 1) * 4 + 63) & ~(size_t)63, o_qb = (o_bases + n_words * 4 + 63) & ~(size_t)63,
                     o_ep = (o_qb + qb + 63) & ~(size_t)63, o_ec = o_ep + n_exc * 4;
        if ((rc = rc_hbuf_reserve(ctx, &sl.p_in, o_ec + n_exc + 64))) return rc;
        char *s = (char *)sl.p_in.p;
        memcpy(s, b->off, (total + 1) * 4);
        memcpy(s + o_bases, b->bases, n_words * 4);
        if (b->qual_bits) memcpy(s + o_qb, b->qual_bits, qb);
        if (n_exc) {
            memcpy(s + o_ep, b->exc_pos, n_exc * 4);
            memcpy(s + o_ec, b->exc_chr, n_exc);
        }
        h_off = (const uint32_t *)s;
        h_bases = (const uint32_t *)(s + o_bases);
        h_qb = b->qual_bits ? (const uint8_t *)(s + o_qb) : nullptr;
        h_exc_pos = (const uint32_t *)(s + o_ep);
        h_exc_chr = (const uint8_t *)(s + o_ec);
    }
    if ((rc = slot_outputs(ctx, sl, rc_slot_out{b->ret, b->l, b->m, b->h, b->fix_pos, b->fix_chr, &b->n_fix}, total, cap))) return rc;
    drain_on_error guard{ctx};
    uint32_t *d_exc_pos = (uint32_t *)sl.d_exc.p;
    uint8_t *d_exc_chr = (uint8_t *)sl.d_exc.p + exc_chr_off;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.d_packed.p, h_bases, n_words * 4, hipMemcpyHostToDevice, ctx->s_h2d));
    if (h_qb) RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.d_qual.p, h_qb, qb, hipMemcpyHostToDevice, ctx->s_h2d));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.d_off.p, h_off, (total + 1) * 4, hipMemcpyHostToDevice, ctx->s_h2d));
    if (n_exc) {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(d_exc_pos, h_exc_pos, n_exc * 4, hipMemcpyHostToDevice, ctx->s_h2d));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(d_exc_chr, h_exc_chr, n_exc, hipMemcpyHostToDevice, ctx->s_h2d));
    }
    RC_CHECK_HIP(ctx, hipEventRecord(sl.e_h2d, ctx->s_h2d));
    // kernels: expand, correct, list the substitutions
    RC_CHECK_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl.e_h2d, 0));
    uint8_t *d_seq = (uint8_t *)sl.d_seq.p;
    if ((rc = rc_launch_unpack(ctx, (const uint32_t *)sl.d_packed.p, nbytes, (const uint32_t *)sl.d_off.p, (uint32_t)total, d_exc_pos, d_exc_chr,
                               (uint32_t)n_exc, d_seq)))
        return rc;
    if (!h_qb) RC_CHECK_HIP(ctx, hipMemsetAsync(sl.d_qual.p, 0, nbytes, ctx->stream));  // FASTA: qual[0] == 0 (Reads.h:224-266)
    const rc_device_batch db = rc_device_batch_over(b->mode, total, nbytes, max_len, d_seq, (const uint8_t *)sl.d_qual.p, (const uint32_t *)sl.d_off.p,
                                                    (int32_t *)sl.d_res.p);
    // (the correction report: staged, the wait decides whether this submission is the one that counts)
    if ((rc = rc_correct_observed(ctx, &db, 0xFFFFFFFFu, 0, h_qb ? 1 : 0, &sl.obs, true))) return rc;
    uint32_t *d_fix_pos, *d_nfix = (uint32_t *)sl.d_fix.p;
    uint8_t *d_fix_chr;
    if ((rc = slot_fix_list_target(ctx, sl, &d_fix_pos, &d_fix_chr))) return rc;
    if ((rc = rc_launch_fix_list(ctx, (const uint32_t *)sl.d_packed.p, nbytes, d_seq, d_exc_pos, (uint32_t)n_exc, d_nfix, cap, d_fix_pos, d_fix_chr))) return rc;
    // the fix count, then the results; the list itself is in host memory by then, rc_wait_packed learns its length
    rc = slot_download(ctx, sl, true, [&]() -> int {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.p_nfix.p, d_nfix, 4, hipMemcpyDeviceToHost, ctx->s_d2h));
        return RC_OK;
    });
    if (rc) return rc;
    guard.armed = false;
    sl.kind = RC_SLOT_PACKED;
    return RC_OK;
}

// ---- the resident transport --------------------------------------------------------------------------
static int submit_resident(rc_ctx_full *ctx, rc_resident_batch *b, int slot)
{
    if (b->mode < 0 || b->mode > 2 || (b->n && (!b->off || !b->ret || !b->l || !b->m || !b->h)) || (b->fix_cap && (!b->fix_pos || !b->fix_chr))) {
        rc_set_error(ctx, "submit_resident: bad batch descriptor");
        return RC_ERR_ARG;
    }
    rc_slot *slp;
    int rc = slot_acquire(ctx, slot, "submit_resident", "wait for it", &slp);
    if (rc) return rc;
    rc_slot &sl = *slp;
    const size_t total = b->mode == 1 ? 2 * b->n : b->n;
    const uint64_t bytes_b = b->mode == 1 ? b->bytes_b : 0;
    const size_t nbytes = (size_t)(b->bytes_a + bytes_b);
    b->n_fix = 0;
    if (total == 0) {
        sl.total_reads = 0;
        sl.kind = RC_SLOT_RESIDENT;
        return RC_OK;
    }
    if (b->bytes_a + bytes_b >= (1ull << 32) || total >= (1ull << 32) || b->fix_cap >= (1ull << 32)) {
        rc_set_error(ctx, "submit_resident: batch too large (split it)");
        return RC_ERR_ARG;
    }
    if (b->mode != 0 && (total & 1)) {
        rc_set_error(ctx, "submit_resident: %s mode needs an even number of reads", b->mode == 1 ? "paired" : "interleaved");
        return RC_ERR_ARG;
    }
    const size_t n_kept = ctx->kept.arenas.size();
    auto in_range = [&](int idx, uint64_t begin, uint64_t bytes) {
        return idx >= 0 && (size_t)idx < n_kept && begin <= ctx->kept.arenas[(size_t)idx].bytes && bytes <= ctx->kept.arenas[(size_t)idx].bytes - begin;
    };
    if (!in_range(b->arena_a, b->begin_a, b->bytes_a) || (b->mode == 1 && !in_range(b->arena_b, b->begin_b, b->bytes_b))) {
        rc_set_error(ctx, "submit_resident: no such range of a kept arena (%zu kept; rc_table_count_keep before counting)", n_kept);
        return RC_ERR_ARG;
    }
    int max_len;
    if ((rc = slot_check_offsets(ctx, "submit_resident", b->off, total, nbytes, b->mode != 1 || b->off[b->n] == b->bytes_a,
                                 "submit_resident: the offsets do not describe the ranges (off[0] = %u, off[%zu] = %u, %zu bytes)", &max_len)))
        return rc;
    sl.total_reads = total;
    const size_t qb = (nbytes + 7) / 8;
    const uint32_t cap = (uint32_t)b->fix_cap;
    sl.arena_bytes = nbytes;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_seq, ((nbytes + 15) & ~(size_t)15) + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_qual, (b->qual_bits ? qb : nbytes) + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_off, (total + 1) * 4))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_res, total * 16))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &sl.d_fix, 64))) return rc;
    if ((rc = rc_hbuf_reserve(ctx, &sl.p_nfix, 64))) return rc;
    const bool in_pinned = rc_is_pinned(b->off, (total + 1) * 4) && (!b->qual_bits || rc_is_pinned(b->qual_bits, qb));
    const uint32_t *h_off = b->off;
    const uint8_t *h_qb = b->qual_bits;
    if (!in_pinned) {
        const size_t o_qb = ((total + 1) * 4 + 63) & ~(size_t)63;
        if ((rc = rc_hbuf_reserve(ctx, &sl.p_in, o_qb + qb + 64))) return rc;
        char *s = (char *)sl.p_in.p;
        memcpy(s, b->off, (total + 1) * 4);
        if (b->qual_bits) memcpy(s + o_qb, b->qual_bits, qb);
        h_off = (const uint32_t *)s;
        h_qb = b->qual_bits ? (const uint8_t *)(s + o_qb) : nullptr;
    }
    if ((rc = slot_outputs(ctx, sl, rc_slot_out{b->ret, b->l, b->m, b->h, b->fix_pos, b->fix_chr, &b->n_fix}, total, cap))) return rc;
    drain_on_error guard{ctx};
    if (h_qb) RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.d_qual.p, h_qb, qb, hipMemcpyHostToDevice, ctx->s_h2d));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.d_off.p, h_off, (total + 1) * 4, hipMemcpyHostToDevice, ctx->s_h2d));
    RC_CHECK_HIP(ctx, hipEventRecord(sl.e_h2d, ctx->s_h2d));
    RC_CHECK_HIP(ctx, hipStreamWaitEvent(ctx->stream, sl.e_h2d, 0));
    // the batch's own arena: its ranges of the kept arenas, side by side
    uint8_t *d_seq = (uint8_t *)sl.d_seq.p;
    const uint8_t *orig_a = (const uint8_t *)ctx->kept.arenas[(size_t)b->arena_a].p + b->begin_a;
    const uint8_t *orig_b = bytes_b ? (const uint8_t *)ctx->kept.arenas[(size_t)b->arena_b].p + b->begin_b : nullptr;
    if (b->bytes_a) RC_CHECK_HIP(ctx, hipMemcpyAsync(d_seq, orig_a, b->bytes_a, hipMemcpyDeviceToDevice, ctx->stream));
    if (bytes_b) RC_CHECK_HIP(ctx, hipMemcpyAsync(d_seq + b->bytes_a, orig_b, bytes_b, hipMemcpyDeviceToDevice, ctx->stream));
    if (!h_qb) RC_CHECK_HIP(ctx, hipMemsetAsync(sl.d_qual.p, 0, nbytes, ctx->stream));  // FASTA: qual[0] == 0 (Reads.h:224-266)
    const rc_device_batch db = rc_device_batch_over(b->mode, total, nbytes, max_len, d_seq, (const uint8_t *)sl.d_qual.p, (const uint32_t *)sl.d_off.p,
                                                    (int32_t *)sl.d_res.p);
    // (the correction report: staged, the wait decides whether this submission is the one that counts)
    if ((rc = rc_correct_observed(ctx, &db, 0xFFFFFFFFu, 0, h_qb ? 1 : 0, &sl.obs, true))) return rc;
    uint32_t *d_fix_pos, *d_nfix = (uint32_t *)sl.d_fix.p;
    uint8_t *d_fix_chr;
    if ((rc = slot_fix_list_target(ctx, sl, &d_fix_pos, &d_fix_chr))) return rc;
    if ((rc = rc_launch_fix_list_bytes(ctx, orig_a, (size_t)b->bytes_a, orig_b, (size_t)bytes_b, d_seq, d_nfix, cap, d_fix_pos, d_fix_chr))) return rc;
    rc = slot_download(ctx, sl, true, [&]() -> int {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(sl.p_nfix.p, d_nfix, 4, hipMemcpyDeviceToHost, ctx->s_d2h));
        return RC_OK;
    });
    if (rc) return rc;
    guard.armed = false;
    sl.kind = RC_SLOT_RESIDENT;
    return RC_OK;
}

extern "C" {

int rc_hbuf_reserve(rc_ctx *ctx, rc_hbuf *h, size_t bytes)
{
    if (bytes <= h->bytes) return RC_OK;
    if (h->p) (void)hipHostFree(h->p);
    h->p = nullptr;
    h->bytes = 0;
    const size_t want = bytes + bytes / 8 + 4096;
    RC_CHECK_HIP(ctx, hipHostMalloc(&h->p, want, hipHostMallocDefault));
    h->bytes = want;
    return RC_OK;
}

static bool is_pinned_at(const void *p)
{
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory the runtime has never seen
        return false;
    }
    return at.type == hipMemoryTypeHost;
}

// the whole range [p, p + bytes) is page-locked: its first and last byte are (a registration or a
// hipHostMalloc block is one contiguous range, so a buffer that starts and ends inside pinned memory and was
// handed over as one array lies in it -- unless it straddles two separate registrations, which then both
// cover their part)
bool rc_is_pinned(const void *p, size_t bytes)
{
    if (!p) return false;
    if (!is_pinned_at(p)) return false;
    return bytes <= 1 || is_pinned_at(static_cast<const char *>(p) + bytes - 1);
}

int rc_host_alloc(rc_ctx *ctx, size_t bytes, void **out)
{
    if (!ctx || !out) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    RC_CHECK_HIP(ctx, hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault));
    return RC_OK;
}

int rc_host_free(rc_ctx *ctx, void *p)
{
    if (!ctx) return RC_ERR_ARG;
    if (p) RC_CHECK_HIP(ctx, hipHostFree(p));
    return RC_OK;
}

// page-locks caller memory (any allocation, whole pages) so that rc_submit can DMA straight from / to it
int rc_host_register(void *p, size_t bytes)
{
    if (!p || !bytes) return RC_ERR_ARG;
    return hipHostRegister(p, bytes, hipHostRegisterPortable) == hipSuccess ? RC_OK : RC_ERR_HIP;
}

int rc_host_unregister(void *p)
{
    if (!p) return RC_ERR_ARG;
    return hipHostUnregister(p) == hipSuccess ? RC_OK : RC_ERR_HIP;
}

int rc_slots_init(rc_ctx *ctx)
{
    if (ctx->slots) return RC_OK;
    RC_CHECK_HIP(ctx, hipStreamCreateWithFlags(&ctx->s_h2d, hipStreamNonBlocking));
    RC_CHECK_HIP(ctx, hipStreamCreateWithFlags(&ctx->s_d2h, hipStreamNonBlocking));
    ctx->slots = new (std::nothrow) rc_slot[RC_MAX_SLOTS];
    if (!ctx->slots) return RC_ERR_NOMEM;
    for (int i = 0; i < RC_MAX_SLOTS; ++i) {
        rc_slot &sl = ctx->slots[i];
        RC_CHECK_HIP(ctx, hipEventCreateWithFlags(&sl.e_h2d, hipEventDisableTiming));
        RC_CHECK_HIP(ctx, hipEventCreateWithFlags(&sl.e_k, hipEventDisableTiming));
        RC_CHECK_HIP(ctx, hipEventCreateWithFlags(&sl.e_done, hipEventDisableTiming));
    }
    return RC_OK;
}

// ---- the entry points ------------------------------------------------------------------------------
int rc_submit(rc_ctx *c, const rc_batch *b, int slot)
{
    if (!b) return RC_ERR_ARG;
    return in_slot_lane(c, slot, true, [b](rc_ctx_full *ctx, int s) { return submit_bytes(ctx, b, s); });
}

int rc_wait(rc_ctx *c, int slot)
{
    return in_slot_lane(c, slot, false, wait_bytes);
}

int rc_submit_packed(rc_ctx *c, rc_packed_batch *b, int slot)
{
    if (!b) return RC_ERR_ARG;
    return in_slot_lane(c, slot, true, [b](rc_ctx_full *ctx, int s) { return submit_packed(ctx, b, s); });
}

int rc_wait_packed(rc_ctx *c, int slot)
{
    return in_slot_lane(c, slot, false, [](rc_ctx_full *ctx, int s) {
        rc_slot *sl = slot_take(ctx, s, RC_SLOT_PACKED, "wait_packed", "packed ");
        return sl ? slot_wait_fix_list(ctx, *sl, "wait_packed") : (int)RC_ERR_STATE;
    });
}

int rc_submit_resident(rc_ctx *c, rc_resident_batch *b, int slot)
{
    if (!b) return RC_ERR_ARG;
    return in_slot_lane(c, slot, true, [b](rc_ctx_full *ctx, int s) { return submit_resident(ctx, b, s); });
}

int rc_wait_resident(rc_ctx *c, int slot)
{
    return in_slot_lane(c, slot, false, [](rc_ctx_full *ctx, int s) {
        rc_slot *sl = slot_take(ctx, s, RC_SLOT_RESIDENT, "wait_resident", "resident ");
        return sl ? slot_wait_fix_list(ctx, *sl, "wait_resident") : (int)RC_ERR_STATE;
    });
}

// ---- the packed boundary's host side: 2-bit bases from a byte arena, a fix list into one ------------
size_t rc_pack_bases(const char *seq, size_t begin, size_t end, uint32_t *bases, uint32_t *exc_pos, uint8_t *exc_chr, size_t exc_cap)
{
    // letter -> code: A0 C1 G2 T3, 4 = NUL, 5 = anything else
    static const struct lut {
        uint8_t v[256];
        lut()
        {
            for (int i = 0; i < 256; ++i) v[i] = 5;
            v[0] = 4;
            v[(int)'A'] = 0;
            v[(int)'C'] = 1;
            v[(int)'G'] = 2;
            v[(int)'T'] = 3;
        }
    } L;
    size_t n_exc = 0;
    const unsigned char *s = reinterpret_cast<const unsigned char *>(seq);
    for (size_t w = begin >> 4; (w << 4) < end; ++w) {
        const size_t p0 = w << 4, lo = p0 < begin ? begin : p0, hi = p0 + 16 > end ? end : p0 + 16;
        uint32_t word = 0;
        for (size_t p = lo; p < hi; ++p) {
            const uint8_t c = L.v[s[p]];
            if (c < 4) {
                word |= (uint32_t)c << (30 - 2 * (p & 15));
            } else if (c == 5) {
                if (n_exc < exc_cap) {
                    exc_pos[n_exc] = (uint32_t)p;
                    exc_chr[n_exc] = s[p];
                }
                ++n_exc;
            }
        }
        // a range that starts inside a word keeps the bits of the positions in front of it (the caller packed them first)
        if (lo > p0) word |= bases[w] & ~(0xFFFFFFFFu >> (2 * (lo - p0)));
        bases[w] = word;
    }
    return n_exc;
}

void rc_apply_fixes(char *seq, const uint32_t *fix_pos, const uint8_t *fix_chr, size_t n_fix)
{
    for (size_t j = 0; j < n_fix; ++j) seq[fix_pos[j]] = (char)fix_chr[j];
}

}  // extern "C"
