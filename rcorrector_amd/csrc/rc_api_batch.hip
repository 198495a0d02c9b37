// rc_api_batch.hip -- C ABI, the correction entry points (include/rcorrector_amd.h): HBM-resident batches and host batches
// (synchronous, traced, per read).  The asynchronous slot transports are rc_api_slots.hip's.
#include "rc_api_internal.h"

extern "C" {

// ---- correction ------------------------------------------------------------------------------
int rc_probe_device(rc_ctx *ctx, const uint8_t *d_seq, uint64_t nbytes, int32_t *d_counts)
{
    if (!ctx || !d_seq || !d_counts) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_probe(ctx, d_seq, (size_t)nbytes, d_counts);
}


// rc_correct_device has no wait: the batch is observed and completes within the call (rc_api_observe.hip), which returns when
// the census and the profile have it; the report counts at the end of the call, in stream order
int rc_correct_device(rc_ctx *ctx, const rc_device_batch *b)
{
    if (!ctx || !b) return RC_ERR_ARG;
    if (const int rc = rc_correct_observed(ctx, b, 0xFFFFFFFFu, 0, -1, &ctx->obs, false)) return rc;
    return rc_batch_completed(ctx, &ctx->obs, nullptr, 0);
}

// what no correction entry point accepts of a batch descriptor with reads in it, refused before anything is launched
int rc_correct_check(rc_ctx *ctx, const rc_device_batch *b)
{
    if (b->mode < 0 || b->mode > 2 || !b->d_seq || !b->d_qual || !b->d_off || !b->d_ret || !b->d_l || !b->d_m || !b->d_h) {
        rc_set_error(ctx, "correct_device: bad batch descriptor");
        return RC_ERR_ARG;
    }
    if (b->nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "correct_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)b->nbytes);
        return RC_ERR_ARG;
    }
    // fill_args refuses such a batch too, but only when a kernel is launched with the batch's own max_len: in a tiered batch
    // that is the long tier's pass, after the short and the middle tier have been corrected in place
    if (b->max_read_len >= RC_MAX_READ_LENGTH) {
        rc_set_error(ctx, "correct: read of %d bases exceeds the %d-base limit (utils.h:7)", b->max_read_len, RC_MAX_READ_LENGTH - 1);
        return RC_ERR_ARG;
    }
    if (!ctx->d_buckets) {  // (before anything is launched: every probe kernel dereferences the table)
        rc_set_error(ctx, "correct: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    // mates travel together (main.cpp:441, :459-468): an odd read count in a paired or interleaved batch has a
    // read without a mate -- refused before the locality order or the pair exchange of the threshold kernel see it
    if (b->mode != 0 && (b->n_reads & 1u)) {
        rc_set_error(ctx, "correct: %s mode needs an even number of reads (got %u)", b->mode == 1 ? "paired" : "interleaved", b->n_reads);
        return RC_ERR_ARG;
    }
    return RC_OK;
}

// ---- the chunked pipeline ---------------------------------------------------------------------------------------------------
// A whole, locality-ordered batch whose reads fit the fused probe + threshold kernel, cut into C chunks of whole tiles of the
// locality list: the fused kernel is launched once per chunk on ctx->stream, and behind each launch the follower stream
// (ctx->stream2) runs that chunk's compaction of the candidates, k_single, compaction of the classes and k_correct -- while the
// fused kernel of the next chunks runs.  The fused kernel waits for memory (its probes) most of its life, k_single and k_correct
// for their vector units.  *ran = false and nothing launched: the batch does not qualify, the caller runs it whole.
//
// What makes the two streams independent between a chunk's fork and the join:
//  * a unit's mates share a tile, hence a chunk: the threshold exchange inside the fused kernel, k_single's and k_correct's
//    strong[mate] / info[mate] never leave the chunk;
//  * the fused kernel of chunk c' WRITES, of per-read state, only that of chunk c''s reads: counts (the reads' own k-mer positions;
//    the up to three words it writes in front of and behind them are positions that hold no count, of any read), strong, info,
//    cls, cand, runs, ret / l / m / h -- and READS the bases of its own reads only (rc_tile_copy_reads loads whole dwords and masks
//    the neighbours' bytes, which k_single / k_correct of another chunk may be rewriting: never used);
//  * the follower's kernels read and write the per-read state of chunk c's reads (c < c'), and what they share among themselves
//    -- the two lists, their counters, the queue heads and phase counters in ctx->work, the search stack, the gathered flags --
//    is used by one follower step at a time: stream2 is serial, and every step of chunk c + 1 queues behind chunk c's k_correct;
//  * the fused kernel touches none of those follower-side buffers, and the table is read-only.
// The join: ctx->stream waits for stream2's last step before anything else is queued on it (k_summary first), so whoever orders
// work behind ctx->stream or waits for it sees a finished batch, as before.  Also after an error: what was forked is joined.
#ifndef RC_PIPE_DEFAULT_CHUNKS
#define RC_PIPE_DEFAULT_CHUNKS 0  // chunks of a batch of RC_PIPE_MIN_READS reads or more where RC_PIPELINE_CHUNKS says nothing (0: off;
                                  // profiles/pipeline_chunks_ab.txt: no chunk count gained on any preset)
#endif
#ifndef RC_PIPE_MIN_READS
#define RC_PIPE_MIN_READS (1u << 22)  // below this a batch's kernels are too short to pay C launches of the persistent kernels
#endif
#ifndef RC_PIPE_DEFAULT_GRID_DIV
#define RC_PIPE_DEFAULT_GRID_DIV 1
#endif
static int rc_pipe_chunks(const rc_ctx *ctx, const rc_device_batch_args &a)
{
    if (ctx->env_pipe_chunks >= 0) return ctx->env_pipe_chunks;
    return a.n >= RC_PIPE_MIN_READS ? RC_PIPE_DEFAULT_CHUNKS : 0;
}

static int rc_correct_pipelined(rc_ctx *ctx, const rc_device_batch_args &a, size_t nbytes, int C, bool *ran)
{
    *ran = false;
    uint32_t rpt = 0;
    const uint32_t n_tiles = rc_fused_tiles(ctx, a, &rpt);
    // (the lists need the classification; the traced and the instrumented k_correct are read back by the host step by step)
    if (C < 2 || !n_tiles || !a.ret || ctx->trace_cap != 0 || ctx->env_no_classify || ctx->phase_prof) return RC_OK;
    int rc;
    ctx->work_stride = ((size_t)a.n + 63) & ~(size_t)63;
    // follower-side buffers at their size for the whole batch, before the fork: a reallocation syncs ctx->stream alone
    if ((rc = rc_dbuf_reserve(ctx, &ctx->worklist, ctx->work_stride * RC_WORK_CLASSES * 4 + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->tier_flag, (size_t)a.n + 256))) return rc;
    auto tile_at = [&](int c) { return (uint32_t)((uint64_t)n_tiles * (uint32_t)c / (uint32_t)C); };
    int c_first = -1, c_last = -1;  // (C > tiles: some chunks are empty; they launch nothing)
    for (int c = 0; c < C; ++c)
        if (tile_at(c + 1) > tile_at(c)) {
            if (c_first < 0) c_first = c;
            c_last = c;
        }
    ctx->thr_ready = true;  // (the fused kernel of a read's chunk has run before any follower kernel looks at the read)
    bool forked = false;
    auto chunks = [&]() -> int {
        for (int c = c_first; c <= c_last; ++c) {
            rc_chunk ch;
            ch.st = ctx->stream2;
            ch.tile_lo = tile_at(c);
            ch.tile_hi = tile_at(c + 1);
            if (ch.tile_hi == ch.tile_lo) continue;
            ch.first = c == c_first;
            ch.last = c == c_last;
            ch.grid_div = ctx->env_pipe_grid_div > 0 ? ctx->env_pipe_grid_div : RC_PIPE_DEFAULT_GRID_DIV;
            bool fused = false;
            int e;
            if ((e = rc_launch_probe_threshold_list(ctx, a, nbytes, &fused, &ch))) return e;
            if (!fused || !ctx->cls_ready) {
                rc_set_error(ctx, "correct: internal: the fused kernel refused a chunk of a batch it accepts");
                return RC_ERR_STATE;
            }
            if (!*ran) ++ctx->pipe_batches;  // (rc_debug_pipeline: host integers, nothing on the device knows of them)
            ++ctx->pipe_chunks;
            *ran = true;
            const hipEvent_t ev = ctx->pipe_ev[ctx->pipe_ev_next++ % rc_ctx::RC_PIPE_EVENTS];
            RC_CHECK_HIP(ctx, hipEventRecord(ev, ctx->stream));
            RC_CHECK_HIP(ctx, hipStreamWaitEvent(ctx->stream2, ev, 0));
            forked = true;
            bool single_ran = false;
            if ((e = rc_launch_single(ctx, a, &single_ran, &ch))) return e;
            if ((e = rc_launch_compact_range(ctx, ch.st, (const uint8_t *)ctx->cls.p, ch.lo, ch.hi, (uint32_t *)ctx->worklist.p, ctx->work_stride,
                                             (uint32_t *)((char *)ctx->work.p + RC_WORK_NWORK_OFF))))
                return e;
            if ((e = rc_launch_correct(ctx, a, &ch))) return e;
        }
        return RC_OK;
    };
    rc = chunks();
    if (forked) {
        const hipError_t e1 = hipEventRecord(ctx->pipe_join, ctx->stream2);
        const hipError_t e2 = e1 == hipSuccess ? hipStreamWaitEvent(ctx->stream, ctx->pipe_join, 0) : e1;
        if (e2 != hipSuccess) {
            (void)hipStreamSynchronize(ctx->stream2);  // (no join in stream order: the host waits instead)
            if (!rc) {
                rc_set_error(ctx, "correct: joining the follower stream failed: %s", hipGetErrorString(e2));
                rc = RC_ERR_HIP;
            }
        }
    }
    return rc;
}

// the correction kernels over a batch rc_correct_check has accepted, ctx's device current (rc_correct_observed)
// qual_split / qual_base2 (quality-bit mode only): arena bytes from qual_split on have their bits at
// byte qual_base2 of d_qual -- the second arena of a paired host batch, whose bit array is separate
// qual_bits: -1 = as rc_set_quality_bits says, 0 / 1 = this batch's quality arena holds bytes / bits (the packed boundary)
int rc_correct_device_impl(rc_ctx *ctx, const rc_device_batch *b, uint32_t qual_split, uint32_t qual_base2, int qual_bits)
{
    int rc;
    bool fused = false;  // probe and threshold kernels ran as one
    ctx->routes_state = rc_ctx::RC_ROUTES_FAILED;  // (rc_debug_routes: until the batch has run to its end, cls / cand / runs describe nothing)
    if ((rc = rc_dbuf_reserve(ctx, &ctx->counts, (size_t)b->nbytes * 4 + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->strong, (size_t)b->n_reads * 4 + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->info, (size_t)b->n_reads * 4 + 256))) return rc;
    rc_device_batch_args a;
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
    a.l = b->d_l;
    a.m = b->d_m;
    a.h = b->d_h;
    a.max_len = b->max_read_len;
    // the reads the threshold kernel could not finish, as a work list; isolated substitutions are finished four reads to
    // a wave first (rc_single.h: it clears their cls), what is left is k_correct's list
    bool loc_order_valid = false;  // ctx->loc_list holds this batch's locality order (every read once) and no length tiers are in play
    auto single_and_compact = [&](const rc_device_batch_args &at) -> int {
        if (!ctx->cls_ready) return RC_OK;
        ctx->work_stride = ((size_t)at.n + 63) & ~(size_t)63;
        int e;
        if ((e = rc_dbuf_reserve(ctx, &ctx->worklist, ctx->work_stride * RC_WORK_CLASSES * 4 + 256))) return e;
        bool ran = false;
        if ((e = rc_launch_single(ctx, at, &ran))) return e;
        if (ctx->env_k3_local && loc_order_valid)
            return rc_launch_compact_local(ctx, (const uint8_t *)ctx->cls.p, at.n, (uint32_t *)ctx->worklist.p, ctx->work_stride,
                                           (uint32_t *)((char *)ctx->work.p + RC_WORK_NWORK_OFF));
        return rc_launch_compact(ctx, (const uint8_t *)ctx->cls.p, at.n, (uint32_t *)ctx->worklist.p, ctx->work_stride,
                                 (uint32_t *)((char *)ctx->work.p + RC_WORK_NWORK_OFF));
    };
    // large batches over a table that does not fit the caches are probed in min-hash order (rc_table.hip),
    // so that overlapping reads meet in the L2 / Infinity Cache
    const bool locality = ctx->locality_mode >= 0 && (ctx->locality_mode > 0 || (a.n >= (1u << 18) && ctx->table_bytes > ((size_t)128 << 20))) &&
                          a.max_len + 8 <= 4000;
    // Length tiers.  The reference treats every read of up to 1 023 bases alike (utils.h:7, ErrorCorrection.cpp:682-1480);
    // here the fast kernels -- the fused probe + threshold kernel, k_single, the compiled-for-k k_correct -- hold reads
    // of up to 160 bases, the quarter-wave threshold kernel 320, and the longest read of a batch used to decide for all
    // of them.  A batch with longer reads is now processed in up to three passes over the same arena, one per tier a
    // unit's longer read falls into: S (<= 160 bases), M (the quarter-wave layout: <= 320 bases / 256 k-mers), L (the
    // rest); each pass = threshold kernel -> (k_single) -> compaction -> k_correct with the tier's capacity class, and the
    // threshold kernel of a pass marks the other tiers' reads cls = 0.  Same results (a read's result depends on its unit
    // alone), the short reads of a mixed batch keep their kernels.  Needs the classification (work lists).
    const int S_HI = 160;
    const int m_hi = RC_Q_MAX_KCNT - 1 + ctx->k < RC_Q_MAX_LEN ? RC_Q_MAX_KCNT - 1 + ctx->k : RC_Q_MAX_LEN;
    const bool tiered = a.max_len > S_HI && !ctx->env_no_tier && !ctx->env_no_classify && !ctx->env_k2_wave_per_read && ctx->trace_cap == 0;
    if (tiered) {
        rc_device_batch_args at = a;
        at.tier_lo = -1;
        at.tier_hi = S_HI;
        at.max_len = S_HI;
        bool lists = false;  // the middle / long tier's reads as lists in locality order (rc_launch_tier_lists)
        if (locality) {
            if ((rc = rc_launch_locality_order(ctx, a, (size_t)b->nbytes))) return rc;
            if ((rc = rc_launch_probe_threshold_list(ctx, at, (size_t)b->nbytes, &fused))) return rc;
            if (fused) {
                // the other tiers' reads are a few per cent of a typical mixed batch: probed (and, the middle tier,
                // thresholded) through compact lists -- walking the whole batch for them cost 3.7 + 3.1 ms of a 25 M-read step
                rc_device_batch_args al = a;
                if ((rc = rc_launch_tier_lists(ctx, a, S_HI, m_hi))) return rc;
                al.max_len = a.max_len < m_hi ? a.max_len : m_hi;
                if ((rc = rc_launch_probe_tier(ctx, al, (size_t)b->nbytes, (int32_t *)ctx->counts.p, 0))) return rc;
                al.max_len = a.max_len;
                if (a.max_len > m_hi && (rc = rc_launch_probe_tier(ctx, al, (size_t)b->nbytes, (int32_t *)ctx->counts.p, 1))) return rc;
                lists = true;
            } else if ((rc = rc_launch_probe_list(ctx, a, (size_t)b->nbytes, (int32_t *)ctx->counts.p, -1)))
                return rc;
        } else if ((rc = rc_launch_probe(ctx, b->d_seq, (size_t)b->nbytes, (int32_t *)ctx->counts.p)))
            return rc;
        ctx->thr_ready = true;  // every pass runs a threshold kernel: k_correct never computes a threshold itself
        for (int tier = 0; tier < 3; ++tier) {
            if (tier == 1) {
                at.tier_lo = S_HI;
                at.tier_hi = m_hi;
                at.max_len = a.max_len < m_hi ? a.max_len : m_hi;
                if (lists) {
                    at.tier_list = (const uint32_t *)ctx->tier_list.p;
                    at.tier_n = (const uint32_t *)((char *)ctx->work.p + RC_WORK_NTIER_OFF);
                }
            } else if (tier == 2) {
                if (a.max_len <= m_hi) break;
                at.tier_lo = m_hi;
                at.tier_hi = RC_TIER_ALL;
                at.max_len = a.max_len;
                at.tier_list = at.tier_n = nullptr;  // (the wave-per-read threshold kernel walks the batch)
            }
            if (!(tier == 0 && fused) && (rc = rc_launch_threshold(ctx, at, true))) return rc;
            if (!ctx->cls_ready) {
                rc_set_error(ctx, "correct: internal: a length tier ran without classification");
                return RC_ERR_STATE;
            }
            if ((rc = single_and_compact(at))) return rc;
            if ((rc = rc_launch_correct(ctx, at))) return rc;
        }
        if ((rc = rc_launch_summary(ctx, a.ret, a.n))) return rc;
        ctx->routes_state = rc_ctx::RC_ROUTES_TIERED;
        return RC_OK;
    }
    if (locality) {
        if ((rc = rc_launch_locality_order(ctx, a, (size_t)b->nbytes))) return rc;
        loc_order_valid = true;
        // the chunked pipeline where it is switched on and the batch qualifies (RC_EXP_PROBE_ONLY builds: never)
#ifndef RC_EXP_PROBE_ONLY
        bool piped = false;
        if ((rc = rc_correct_pipelined(ctx, a, (size_t)b->nbytes, rc_pipe_chunks(ctx, a), &piped))) return rc;
        if (piped) {
            if ((rc = rc_launch_summary(ctx, a.ret, a.n))) return rc;
            ctx->routes_state = rc_ctx::RC_ROUTES_WHOLE;
            ctx->routes_n = a.n;
            return RC_OK;
        }
#endif
        // probe + threshold + classification in one kernel where the reads fit it
        if ((rc = rc_launch_probe_threshold_list(ctx, a, (size_t)b->nbytes, &fused))) return rc;
        if (!fused && (rc = rc_launch_probe_list(ctx, a, (size_t)b->nbytes, (int32_t *)ctx->counts.p))) return rc;
    } else if ((rc = rc_launch_probe(ctx, b->d_seq, (size_t)b->nbytes, (int32_t *)ctx->counts.p)))
        return rc;
#ifdef RC_EXP_PROBE_ONLY  // dev (with RC_EXP_ADDR_WINDOW, whose counts are wrong by design): nothing behind the probe kernel runs
    return RC_OK;
#endif
    // thresholds: mates need each other's before either can be corrected, so paired / interleaved
    // batches always run the threshold kernel first; single-end batches do too when every read fits
    // the four-reads-per-wave kernel (cheaper there than inside k_correct), else k_correct computes them
    ctx->thr_ready = fused;
    if (!fused) ctx->cls_ready = false;
    const bool quarter_ok = a.max_len <= 320 && a.max_len - ctx->k + 1 <= 256 && !ctx->env_k2_wave_per_read;
    if (!fused && (a.mode != 0 || quarter_ok)) {
        if ((rc = rc_launch_threshold(ctx, a, true))) return rc;
        ctx->thr_ready = true;
    }
    if ((rc = single_and_compact(a))) return rc;
    if ((rc = rc_launch_correct(ctx, a))) return rc;
    // UpdateSummary (main.cpp:73-79), on the device: the counters live in HBM until rc_summary() asks
    if ((rc = rc_launch_summary(ctx, a.ret, a.n))) return rc;
    ctx->routes_state = rc_ctx::RC_ROUTES_WHOLE;
    ctx->routes_n = a.n;
    return RC_OK;
}

// GetStrongTrustedThreshold (ErrorCorrection.h:26, ErrorCorrection.cpp:1482-1565) for every read of
// an arena in HBM: probe kernel + threshold kernel, the per-read values copied to d_strong
int rc_strong_threshold_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                               int32_t max_read_len, int32_t *d_strong)
{
    if (!ctx || !d_seq || !d_off || !d_strong) return RC_ERR_ARG;
    if (n_reads == 0) return RC_OK;
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "strong_threshold_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->counts, (size_t)nbytes * 4 + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->strong, (size_t)n_reads * 4 + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->info, (size_t)n_reads * 4 + 256))) return rc;
    rc_device_batch_args a = rc_device_batch_args();  // (value-initialised: zeros, and the members with defaults -- no tiers)
    a.mode = 0;
    a.n = n_reads;
    a.seq = const_cast<uint8_t *>(d_seq);
    a.nbytes = (size_t)nbytes;
    a.off = d_off;
    a.max_len = max_read_len;
    if ((rc = rc_launch_probe(ctx, d_seq, (size_t)nbytes, (int32_t *)ctx->counts.p))) return rc;
    if ((rc = rc_launch_threshold(ctx, a, false))) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(d_strong, ctx->strong.p, (size_t)n_reads * 4, hipMemcpyDeviceToDevice, ctx->stream));
    return RC_OK;
}

// ---- per-read entry points: the granularity of ErrorCorrection.h:26-28, each a batch of one through the kernels above
// (a launch and two copies per call -- for bindings that work read by read and for spot checks, not for throughput)
static int one_read_upload(rc_ctx *ctx, const char *seq, const char *qual, rc_device_batch_args &a, size_t *len1)
{
    if (!seq) return RC_ERR_ARG;
    const size_t n1 = strlen(seq) + 1;
    if (n1 > RC_MAX_READ_LENGTH) {
        rc_set_error(ctx, "read of %zu bases exceeds the %d-base limit (utils.h:7)", n1 - 1, RC_MAX_READ_LENGTH - 1);
        return RC_ERR_ARG;
    }
    if (ctx->qual_bits) {
        rc_set_error(ctx, "the per-read entry points take quality bytes (rc_set_quality_bits is on)");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    int rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->h_seq, n1 + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->h_qual, n1 + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->h_off, 2 * 4))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->h_res, 4 * 4))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->counts, n1 * 4 + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->strong, 4 + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->info, 4 + 256))) return rc;
    const uint32_t off[2] = {0u, (uint32_t)n1};
    RC_CHECK_HIP(ctx, hipMemcpyAsync(ctx->h_seq.p, seq, n1, hipMemcpyHostToDevice, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemsetAsync(ctx->h_qual.p, 0, n1, ctx->stream));  // (no qualities: the FASTA marker qual[0] == 0)
    if (qual) {
        const size_t q1 = strnlen(qual, n1 - 1);
        RC_CHECK_HIP(ctx, hipMemcpyAsync(ctx->h_qual.p, qual, q1, hipMemcpyHostToDevice, ctx->stream));
    }
    RC_CHECK_HIP(ctx, hipMemcpyAsync(ctx->h_off.p, off, sizeof off, hipMemcpyHostToDevice, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (off and possibly seq are on the caller's stack)
    int32_t *d_res = (int32_t *)ctx->h_res.p;
    a = rc_device_batch_args();
    a.mode = 0;
    a.n = 1;
    a.seq = (uint8_t *)ctx->h_seq.p;
    a.nbytes = n1;
    a.qual = (const uint8_t *)ctx->h_qual.p;
    a.off = (const uint32_t *)ctx->h_off.p;
    a.ret = d_res;
    a.l = d_res + 1;
    a.m = d_res + 2;
    a.h = d_res + 3;
    a.max_len = (int)n1 - 1;
    *len1 = n1;
    return RC_OK;
}

int rc_strong_threshold_read(rc_ctx *ctx, const char *seq, int32_t *strong)
{
    if (!ctx || !seq || !strong) return RC_ERR_ARG;
    rc_device_batch_args a;
    size_t n1;
    int rc = one_read_upload(ctx, seq, nullptr, a, &n1);
    if (rc) return rc;
    if ((rc = rc_launch_probe(ctx, a.seq, n1, (int32_t *)ctx->counts.p))) return rc;
    if ((rc = rc_launch_threshold(ctx, a, false))) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(strong, ctx->strong.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

int rc_correct_read(rc_ctx *ctx, char *seq, const char *qual, int32_t pair_strong_threshold, int32_t *ret)
{
    if (!ctx || !seq || !ret) return RC_ERR_ARG;
    rc_device_batch_args a;
    size_t n1;
    int rc = one_read_upload(ctx, seq, qual, a, &n1);
    if (rc) return rc;
    a.pair_override = pair_strong_threshold;
    const uint8_t *snap;  // (the correction report alone: one read is no batch of the run for the other observers)
    if ((rc = rc_report_snapshot(ctx, a.seq, n1, false, &snap))) return rc;
    if ((rc = rc_launch_probe(ctx, a.seq, n1, (int32_t *)ctx->counts.p))) return rc;
    // no threshold kernel, no classification: k_correct computes the read's own threshold (its single-end front end) and
    // takes the pair's from the argument, exactly the reference's call
    ctx->thr_ready = false;
    ctx->cls_ready = false;
    ctx->cand_ready = false;
    if ((rc = rc_launch_correct(ctx, a))) return rc;
    if ((rc = rc_launch_summary(ctx, a.ret, 1))) return rc;
    const rc_device_batch db = rc_device_batch_over(0, 1, n1, a.max_len, a.seq, a.qual, a.off, a.ret);  // (one_read_upload: a.ret | l | m | h is one block)
    if ((rc = rc_report_count(ctx, &db, 0xFFFFFFFFu, 0, 0, snap, nullptr))) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(seq, a.seq, n1 - 1, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(ret, a.ret, 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

int rc_kmer_info_read(rc_ctx *ctx, const char *seq, int32_t *l, int32_t *m, int32_t *h)
{
    if (!ctx || !seq || !l || !m || !h) return RC_ERR_ARG;
    rc_device_batch_args a;
    size_t n1;
    int rc = one_read_upload(ctx, seq, nullptr, a, &n1);
    if (rc) return rc;
    if ((rc = rc_launch_probe(ctx, a.seq, n1, (int32_t *)ctx->counts.p))) return rc;
    if ((rc = rc_launch_kmer_info(ctx, a))) return rc;
    int32_t out[3];
    RC_CHECK_HIP(ctx, hipMemcpyAsync(out, a.l, 12, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *l = out[0];
    *m = out[1];
    *h = out[2];
    return RC_OK;
}

int rc_sync(rc_ctx *ctx)
{
    return ctx ? rc_drain(ctx) : (int)RC_ERR_ARG;
}

static int correct_batch_impl(rc_ctx *c, rc_batch *b, rc_trace *t);

int rc_submit(rc_ctx *c, const rc_batch *b, int slot);
int rc_wait(rc_ctx *c, int slot);

int rc_correct_batch(rc_ctx *c, rc_batch *b)
{
    int rc = rc_submit(c, b, 0);
    if (rc) return rc;
    return rc_wait(c, 0);
}

// rc_correct_batch + what the reference prints under -verbose (VERBOSE, ErrorCorrection.cpp:15):
// the counts before (:759-770) and after (:1590-1597) come from two extra runs of the probe
// kernel, the per-iteration thresholds and bitmaps (:856-857, :1088-1094) from the TRACE build of
// k_correct
int rc_correct_batch_traced(rc_ctx *c, rc_batch *b, rc_trace *t)
{
    if (!c || !b || !t) return RC_ERR_ARG;
    if (t->max_iter < 1 || !t->counts_before || !t->counts_after || !t->flags || !t->n_iter || !t->iter) {
        rc_set_error(c, "correct_batch_traced: bad trace descriptor");
        return RC_ERR_ARG;
    }
    if (c->qual_bits) {
        rc_set_error(c, "correct_batch_traced: not available in quality-bit mode");
        return RC_ERR_STATE;
    }
    c->trace_cap = t->max_iter;
    int rc = correct_batch_impl(c, b, t);
    c->trace_cap = 0;
    return rc;
}

static int correct_batch_impl(rc_ctx *c, rc_batch *b, rc_trace *t)
{
    if (!c || !b) return RC_ERR_ARG;
    rc_ctx_full *ctx = static_cast<rc_ctx_full *>(c);
    if (b->n == 0) return RC_OK;
    if (b->mode < 0 || b->mode > 2 || !b->seq || !b->qual || !b->off || !b->ret || !b->l || !b->m || !b->h ||
        (b->mode == 1 && (!b->seq2 || !b->qual2 || !b->off2))) {
        rc_set_error(ctx, "correct_batch: bad batch descriptor");
        return RC_ERR_ARG;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n1 = b->n;
    const size_t bytes1 = b->off[n1], bytes2 = b->mode == 1 ? b->off2[n1] : 0;
    const size_t total_reads = b->mode == 1 ? 2 * n1 : n1;
    const size_t nbytes = bytes1 + bytes2;
    if (nbytes >= (1ull << 32) || total_reads >= (1ull << 32)) {
        rc_set_error(ctx, "correct_batch: batch too large (split it)");
        return RC_ERR_ARG;
    }
    std::vector<uint32_t> off(total_reads + 1);
    const int max_len = rc_concat_offsets(b, bytes1, off.data());
    int rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->h_seq, nbytes + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->h_qual, nbytes + 64))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->h_off, (total_reads + 1) * 4))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->h_res, total_reads * 16))) return rc;
    uint8_t *d_seq = (uint8_t *)ctx->h_seq.p, *d_qual = (uint8_t *)ctx->h_qual.p;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(d_seq, b->seq, bytes1, hipMemcpyHostToDevice, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(d_qual, b->qual, bytes1, hipMemcpyHostToDevice, ctx->stream));
    if (b->mode == 1) {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(d_seq + bytes1, b->seq2, bytes2, hipMemcpyHostToDevice, ctx->stream));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(d_qual + bytes1, b->qual2, bytes2, hipMemcpyHostToDevice, ctx->stream));
    }
    RC_CHECK_HIP(ctx, hipMemcpyAsync(ctx->h_off.p, off.data(), (total_reads + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    const rc_device_batch db = rc_device_batch_over(b->mode, total_reads, nbytes, max_len, d_seq, d_qual, (const uint32_t *)ctx->h_off.p, (int32_t *)ctx->h_res.p);
    if ((rc = rc_correct_observed(ctx, &db, 0xFFFFFFFFu, 0, -1, &ctx->obs, false))) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(b->seq, d_seq, bytes1, hipMemcpyDeviceToHost, ctx->stream));
    if (b->mode == 1) RC_CHECK_HIP(ctx, hipMemcpyAsync(b->seq2, d_seq + bytes1, bytes2, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(b->ret, db.d_ret, total_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(b->l, db.d_l, total_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(b->m, db.d_m, total_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(b->h, db.d_h, total_reads * 4, hipMemcpyDeviceToHost, ctx->stream));
    if (t) {
        // before: K1's output is still in ctx->counts; after: probe the corrected arena once more
        RC_CHECK_HIP(ctx, hipMemcpyAsync(t->counts_before, ctx->counts.p, nbytes * 4, hipMemcpyDeviceToHost, ctx->stream));
        if ((rc = rc_launch_probe(ctx, d_seq, nbytes, (int32_t *)ctx->counts.p))) return rc;
        RC_CHECK_HIP(ctx, hipMemcpyAsync(t->counts_after, ctx->counts.p, nbytes * 4, hipMemcpyDeviceToHost, ctx->stream));
        const size_t rec = 2 + (size_t)t->max_iter * RC_TRACE_WORDS;
        std::vector<int32_t> raw(total_reads * rec);
        RC_CHECK_HIP(ctx, hipMemcpyAsync(raw.data(), ctx->trace.p, raw.size() * 4, hipMemcpyDeviceToHost, ctx->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < total_reads; ++i) {
            const int32_t *r = raw.data() + i * rec;
            t->flags[i] = r[0];
            t->n_iter[i] = r[1];
            memcpy(t->iter + i * (size_t)t->max_iter * RC_TRACE_WORDS, r + 2, (size_t)t->max_iter * RC_TRACE_WORDS * 4);
        }
    }
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return rc_batch_completed(ctx, &ctx->obs, d_seq, nbytes);  // (the traced entry point's batches complete here)
}

}  // extern "C"
