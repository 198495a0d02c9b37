// rc_api_trust.hip -- C ABI, the k-mer trust profile by read position (include/rcorrector_amd.h: rc_trust_profile; kernels in
// rc_trust.hip): the device entry point, opening, reading and closing a profile, and the two steps the correction entry points
// take for it.
//
// Where the counts go: a batch's BEFORE counts are taken on the stream of the context it runs in once its bases are in HBM
// and before the first correction kernel, its AFTER counts behind the last one (rc_trust_stage), both into an rc_trust_counts
// pair of the slot (or of the context, for the entry points that have no slot), zeroed first.  They are added to the profile
// when the batch completes (rc_trust_commit) -- once, however often a batch that did not fit its fix list was submitted.  Both
// steps are called from one place each, rc_correct_observed and rc_batch_completed (rc_api_observe.hip), which say where they
// sit for every entry point.  Slot lanes are contexts on streams of their own: they add to the profile of the context they serve
// under its obs_mutex, and a commit is complete on return, so two lanes never add at once and a slot's pair is free again.
#include "rc_api_internal.h"

#include <cstddef>

#include "rc_trust.h"

#define RC_TRUST_WORDS (sizeof(rc_trust_counts) / 8)  // 64-bit counts of one version
static_assert(RC_TRUST_MAX_LEN == RC_TRUST_LEN, "rc_trust.h's positions are the header's");
static_assert(sizeof(rc_trust_counts) == 5 * 2 * RC_TRUST_MAX_LEN * 8, "five arrays of [2][RC_TRUST_MAX_LEN], as k_trust_reduce indexes them");
static_assert(offsetof(rc_trust_counts, windows) == 0 && offsetof(rc_trust_counts, solid5) == 2 * RC_TRUST_MAX_LEN * 8 &&
                  offsetof(rc_trust_counts, weak5) == 4 * RC_TRUST_MAX_LEN * 8 && offsetof(rc_trust_counts, solid3) == 6 * RC_TRUST_MAX_LEN * 8 &&
                  offsetof(rc_trust_counts, weak3) == 8 * RC_TRUST_MAX_LEN * 8,
              "windows, solid5, weak5, solid3, weak3");
static_assert(offsetof(rc_trust_profile, after) == offsetof(rc_trust_profile, before) + sizeof(rc_trust_counts), "before | after, as in HBM");

extern "C" {

int rc_trust_stage(rc_ctx *ctx, const rc_device_batch *b, int version, rc_trust_staged *st)
{
    if (version == 0) {
        st->staged = false;
        rc_ctx *home = rc_home(ctx);
        if (!home->trust_open) return RC_OK;
        if (const int rc = rc_dbuf_reserve(ctx, &st->buf, 2 * sizeof(rc_trust_counts))) return rc;
        RC_CHECK_HIP(ctx, hipMemsetAsync(st->buf.p, 0, 2 * sizeof(rc_trust_counts), ctx->stream));
        st->gen = home->trust_gen;
        st->min_count = home->trust_min;
        st->n_reads = b->n_reads;
        st->mode = b->mode;
        st->max_read_len = std::min(b->max_read_len, RC_TRUST_MAX_LEN - 1);
        if (const int rc = rc_launch_trust_profile(ctx, b->d_seq, (size_t)b->nbytes, b->d_off, b->n_reads, st->max_read_len, b->mode, st->min_count,
                                                   &ctx->trust_planes, &ctx->trust_part, st->buf.p))
            return rc;
        st->staged = true;
        return RC_OK;
    }
    if (!st->staged) return RC_OK;  // (no profile was open when the batch's bases arrived: it is in none)
    return rc_launch_trust_profile(ctx, b->d_seq, (size_t)b->nbytes, b->d_off, b->n_reads, st->max_read_len, b->mode, st->min_count, &ctx->trust_planes,
                                   &ctx->trust_part, (char *)st->buf.p + sizeof(rc_trust_counts));
}

int rc_trust_commit(rc_ctx *ctx, rc_trust_staged *st)
{
    if (!st->staged) return RC_OK;
    st->staged = false;
    rc_ctx *home = rc_home(ctx);
    std::lock_guard<std::mutex> lk(home->obs_mutex);
    if (!home->trust_open || home->trust_gen != st->gen) return RC_OK;  // (staged for a profile that has ended)
    if (const int rc = rc_launch_trust_add(ctx, st->buf.p, home->trust_acc, (uint32_t)(2 * RC_TRUST_WORDS))) return rc;
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (st->mode == 0) {
        home->trust_reads[0] += st->n_reads;
    } else {
        home->trust_reads[0] += st->n_reads >> 1;
        home->trust_reads[1] += st->n_reads >> 1;
    }
    return RC_OK;
}

static void trust_release(rc_ctx *ctx)
{
    if (ctx->trust_acc) (void)hipFree(ctx->trust_acc);
    ctx->trust_acc = nullptr;
    ctx->trust_open = false;
    auto scratch = [](rc_ctx *c) {
        if (!c) return;
        for (rc_dbuf *b : {&c->trust_planes, &c->trust_part}) {
            if (b->p) (void)hipFree(b->p);
            *b = rc_dbuf();
        }
    };
    scratch(ctx);
    for (rc_ctx *ln : ctx->lane) scratch(ln);
    rc_observed_drop_all(ctx, RC_OBS_TRUST, true);  // (the staged counts of ctx, its lanes and their slots)
}

int rc_trust_profile_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes, int32_t max_read_len,
                            int32_t mode, int32_t min_count, rc_trust_counts *d_counts)
{
    if (!ctx) return RC_ERR_ARG;
    if (min_count < 1) {
        rc_set_error(ctx, "trust_profile_device: min_count must be at least 1 (got %d)", min_count);
        return RC_ERR_ARG;
    }
    if (mode < 0 || mode > 2) {
        rc_set_error(ctx, "trust_profile_device: mode must be 0, 1 or 2 (got %d)", mode);
        return RC_ERR_ARG;
    }
    if (mode == 1 && (n_reads & 1u)) {
        rc_set_error(ctx, "trust_profile_device: paired mode needs an even number of reads (got %u)", n_reads);
        return RC_ERR_ARG;
    }
    if (n_reads && (!d_seq || !d_off || !d_counts)) {
        rc_set_error(ctx, "trust_profile_device: null pointer");
        return RC_ERR_ARG;
    }
    if (max_read_len > RC_TRUST_MAX_LEN - 1) {
        rc_set_error(ctx, "trust_profile_device: max_read_len %d: a profile holds reads of up to %d bases", max_read_len, RC_TRUST_MAX_LEN - 1);
        return RC_ERR_ARG;
    }
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "trust_profile_device: arena of %llu bytes exceeds the 4 GiB batch limit", (unsigned long long)nbytes);
        return RC_ERR_ARG;
    }
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "trust_profile: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    if (n_reads == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_launch_trust_profile(ctx, d_seq, (size_t)nbytes, d_off, n_reads, max_read_len, mode, min_count, &ctx->trust_planes, &ctx->trust_part, d_counts);
}

int rc_trust_profile_begin(rc_ctx *ctx, int32_t min_count)
{
    if (!ctx) return RC_ERR_ARG;
    if (min_count < 1) {
        rc_set_error(ctx, "trust_profile_begin: min_count must be at least 1 (got %d)", min_count);
        return RC_ERR_ARG;
    }
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    if (ctx->trust_open) {
        rc_set_error(ctx, "trust_profile_begin: a profile is open already (rc_trust_profile_end it first)");
        return RC_ERR_STATE;
    }
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "trust_profile_begin: no k-mer table loaded (min_count means nothing without one)");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    RC_CHECK_HIP(ctx, hipMalloc(&ctx->trust_acc, 2 * sizeof(rc_trust_counts)));
    if (hipMemset(ctx->trust_acc, 0, 2 * sizeof(rc_trust_counts)) != hipSuccess) {
        (void)hipFree(ctx->trust_acc);
        ctx->trust_acc = nullptr;
        rc_set_error(ctx, "trust_profile_begin: could not clear the counts");
        return RC_ERR_HIP;
    }
    ctx->trust_reads[0] = ctx->trust_reads[1] = 0;
    ctx->trust_min = min_count;
    ++ctx->trust_gen;
    ctx->trust_open = true;
    return RC_OK;
}

int rc_trust_profile_get(rc_ctx *ctx, rc_trust_profile *out)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->trust_open) {
        rc_set_error(ctx, "trust_profile_get: call rc_trust_profile_begin first");
        return RC_ERR_STATE;
    }
    if (!out) {
        rc_set_error(ctx, "trust_profile_get: out must not be NULL");
        return RC_ERR_ARG;
    }
    if (const int rc = rc_drain(ctx)) return rc;
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    out->k = ctx->k;
    out->min_count = ctx->trust_min;
    out->reads[0] = ctx->trust_reads[0];
    out->reads[1] = ctx->trust_reads[1];
    RC_CHECK_HIP(ctx, hipMemcpy(&out->before, ctx->trust_acc, 2 * sizeof(rc_trust_counts), hipMemcpyDeviceToHost));
    return RC_OK;
}

int rc_trust_profile_end(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->trust_open) {
        rc_set_error(ctx, "trust_profile_end: no profile is open");
        return RC_ERR_STATE;
    }
    const int rc = rc_drain(ctx);  // (a lane's kernels may still write its slot's counts and its scratch)
    std::lock_guard<std::mutex> lk(ctx->obs_mutex);
    trust_release(ctx);
    return rc;
}

}  // extern "C"
