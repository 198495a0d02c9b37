// rc_api_table.hip -- C ABI, the k-mer table and the run parameters (include/rcorrector_amd.h): dump load, GPU counting,
// sharing / replication, lookup / export / digest, ERROR_RATE, bad quality.  Host code only drives HIP.
#include "rc_api_internal.h"

extern "C" {

// ---- table ---------------------------------------------------------------------------------
int rc_table_build_device(rc_ctx *ctx, uint64_t *d_codes, const int32_t *d_counts, size_t n)
{
    if (!ctx) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    static_cast<rc_ctx_full *>(ctx)->dump.valid = false;
    int rc = rc_launch_canonicalize(ctx, d_codes, n);
    if (rc) return rc;
    return rc_build_table_from_device_pairs(ctx, d_codes, d_counts, n);
}

int rc_table_build(rc_ctx *ctx, const uint64_t *codes, const int32_t *counts, size_t n)
{
    if (!ctx || (n && (!codes || !counts))) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    rc_dev_tmp b_codes, b_counts;
    if (n) {
        RC_CHECK_HIP(ctx, b_codes.alloc(n * 8));
        RC_CHECK_HIP(ctx, b_counts.alloc(n * 4));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(b_codes.p, codes, n * 8, hipMemcpyHostToDevice, ctx->stream));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(b_counts.p, counts, n * 4, hipMemcpyHostToDevice, ctx->stream));
    }
    return rc_table_build_device(ctx, b_codes.as<uint64_t>(), b_counts.as<int32_t>(), n);
}

// n x Store::Put in file order: the pieces go to the device one after the other, no host copy
static int dump_upload_and_build(rc_ctx *ctx, const std::vector<rc_dump_piece> &pieces, size_t n_put)
{
    rc_dev_tmp b_codes, b_counts;
    RC_CHECK_HIP(ctx, b_codes.alloc(n_put * 8));
    RC_CHECK_HIP(ctx, b_counts.alloc(n_put * 4));
    size_t at = 0;
    for (const rc_dump_piece &P : pieces) {
        const size_t m = P.put_codes.size();
        if (m) {
            RC_CHECK_HIP(ctx, hipMemcpyAsync(b_codes.as<uint64_t>() + at, P.put_codes.data(), m * 8, hipMemcpyHostToDevice, ctx->stream));
            RC_CHECK_HIP(ctx, hipMemcpyAsync(b_counts.as<int32_t>() + at, P.put_counts.data(), m * 4, hipMemcpyHostToDevice, ctx->stream));
        }
        at += m;
    }
    const int rc = rc_table_build_device(ctx, b_codes.as<uint64_t>(), b_counts.as<int32_t>(), n_put);
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the pieces' host arrays go with the caller's vector)
    return rc;
}

// main.cpp:294-308: the text (rc_jfdump.h) read, parsed on several host threads and joined in file order, then the table
int rc_table_load_jfdump(rc_ctx *c, const char *path, int64_t *stored)
{
    if (!c || !path) return RC_ERR_ARG;
    rc_ctx_full *ctx = static_cast<rc_ctx_full *>(c);
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    rc_dump_text text;
    char err[512];
    if (const int rc = rc_dump_read_file(path, &text, err, sizeof err)) {
        rc_set_error(ctx, "%s", err);
        return rc;
    }
    auto now = []() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t_read = now();
    std::vector<rc_dump_piece> pieces = rc_dump_parse(text.p, text.n, ctx->k, rc_host_threads(text.n, (size_t)1 << 20));
    size_t n_put = 0;
    int64_t accepted = 0;
    rc_dump_join(pieces, &ctx->dump, &n_put, &accepted);  // (dump.valid == false from here until the table stands)
    const double t_parse = now();
    if (stored) *stored = accepted;
    const int rc = dump_upload_and_build(ctx, pieces, n_put);
    if (ctx->env_timing) fprintf(stderr, "[rc timing] dump: parse %.2f s, table build %.2f s\n", t_parse - t_read, now() - t_parse);
    ctx->dump.valid = rc == RC_OK;  // (rc_table_build_device drops the cache of an earlier dump)
    return rc;
}

int rc_table_share(rc_ctx *dst, const rc_ctx *src)
{
    if (!dst || !src || dst == src) return RC_ERR_ARG;
    if (dst->device != src->device || dst->k != src->k) {
        rc_set_error(dst, "table_share: contexts must be on the same device with the same k");
        return RC_ERR_ARG;
    }
    if (!src->d_buckets) {
        rc_set_error(dst, "table_share: the source context has no table");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(dst, hipSetDevice(dst->device));
    rc_table_release(dst);
    dst->table() = src->table();
    dst->buckets_borrowed = true;
    return RC_OK;
}

// the copy itself is queued on dst's stream (rc_sync(dst) waits for it), so that a host replicating to several GPUs
// has all its copies in flight at once: the GPUs of a node are linked pairwise (xGMI), one copy per link
int rc_table_replicate_async(rc_ctx *dst, const rc_ctx *src)
{
    if (!dst || !src || dst == src) return RC_ERR_ARG;
    if (dst->k != src->k) {
        rc_set_error(dst, "table_replicate: contexts must have the same k");
        return RC_ERR_ARG;
    }
    if (!src->d_buckets) {
        rc_set_error(dst, "table_replicate: the source context has no table");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(dst, hipSetDevice(src->device));
    RC_CHECK_HIP(dst, hipStreamSynchronize(src->stream));
    RC_CHECK_HIP(dst, hipSetDevice(dst->device));
    rc_table_release(dst);
    static_cast<rc_ctx_full *>(dst)->dump.valid = false;
    // the new allocation belongs to a guard until every copy is queued: an error on the way leaves dst without a table
    // (d_buckets == nullptr), not with a pointer whose geometry still describes the previous one
    rc_dev_tmp guard;
    const size_t bytes = src->table_bytes + RC_TABLE_PREFIX_BYTES + (size_t)src->filter_words * 4;  // prefix, buckets, filter
    RC_CHECK_HIP(dst, guard.alloc(bytes));
    char *base = guard.as<char>();
    const char *from = reinterpret_cast<const char *>(src->d_buckets) - RC_TABLE_PREFIX_BYTES;
    // the bucket array (and its prefix) is the table
    if (const int rc = rc_copy_across(dst, base, dst->device, from, src->device, bytes, dst->stream, "table_replicate: staged copy")) return rc;
    dst->table() = src->table();
    dst->d_buckets = reinterpret_cast<uint32_t *>(base + RC_TABLE_PREFIX_BYTES);
    guard.p = nullptr;  // (dst owns it now)
    return RC_OK;
}

int rc_table_replicate(rc_ctx *dst, const rc_ctx *src)
{
    int rc = rc_table_replicate_async(dst, src);
    if (rc) return rc;
    RC_CHECK_HIP(dst, hipStreamSynchronize(dst->stream));
    return RC_OK;
}

int rc_table_count_reads_device(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, int min_count, int64_t *n_kmers)
{
    if (!ctx || !d_seq) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    static_cast<rc_ctx_full *>(ctx)->dump.valid = false;
    return rc_count_reads(ctx, d_seq, nbytes, min_count, n_kmers);
}

int rc_table_count_begin(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_count_begin(ctx);
}

int rc_table_count_keep(rc_ctx *ctx, int on)
{
    if (!ctx) return RC_ERR_ARG;
    ctx->cnt_keep = on != 0;
    return RC_OK;
}

int rc_table_count_arenas(const rc_ctx *ctx, size_t *n_arenas, uint64_t *bytes, size_t cap)
{
    if (!ctx || !n_arenas) return RC_ERR_ARG;
    *n_arenas = ctx->kept.arenas.size();
    for (size_t i = 0; bytes && i < cap && i < ctx->kept.arenas.size(); ++i) bytes[i] = ctx->kept.arenas[i].bytes;
    return RC_OK;
}

int rc_table_count_release(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = rc_drain(ctx)) return rc;  // (a batch still reading them, here or in a slot lane)
    for (rc_ctx *ln : ctx->lane)  // the slot lanes hold copies of the descriptors
        if (ln) ln->kept.arenas.clear();
    ctx->kept.release();
    return RC_OK;
}

int rc_table_count_add_device(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes)
{
    if (!ctx || (nbytes && !d_seq)) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_count_add(ctx, d_seq, nbytes, true);
}

int rc_table_count_add(rc_ctx *ctx, const char *seq, size_t nbytes)
{
    if (!ctx || (nbytes && !seq)) return RC_ERR_ARG;
    if (nbytes == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_count_add(ctx, reinterpret_cast<const uint8_t *>(seq), nbytes, false);
}

int rc_table_count_finish(rc_ctx *ctx, int min_count, int64_t *n_kmers)
{
    if (!ctx) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    static_cast<rc_ctx_full *>(ctx)->dump.valid = false;
    return rc_count_finish(ctx, min_count, n_kmers);
}

int rc_table_count_finish_sharded(rc_ctx **ctxs, int n, int min_count, int64_t *n_kmers)
{
    if (!ctxs || n < 1 || !ctxs[0]) return RC_ERR_ARG;
    for (int g = 0; g < n; ++g)
        if (!ctxs[g]) return RC_ERR_ARG;
    if (n == 1) return rc_table_count_finish(ctxs[0], min_count, n_kmers);
    RC_CHECK_HIP(ctxs[0], hipSetDevice(ctxs[0]->device));
    static_cast<rc_ctx_full *>(ctxs[0])->dump.valid = false;
    const int rc = rc_count_finish_sharded(ctxs, n, min_count, n_kmers);
    (void)hipSetDevice(ctxs[0]->device);
    return rc;
}

int rc_table_count_park(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_count_park(ctx);
}

// the table as `jellyfish dump` text (">COUNT\nKMER\n" per entry, canonical k-mer), in dump order
int rc_table_write_jfdump(rc_ctx *ctx, const char *path, int64_t *n_written)
{
    if (!ctx || !path) return RC_ERR_ARG;
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "write_jfdump: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<uint64_t> codes;
    std::vector<int32_t> counts;
    int rc = rc_table_entries_in_dump_order(ctx, &codes, &counts);
    if (rc) return rc;
    FILE *fp = fopen(path, "wb");
    if (!fp) {
        rc_set_error(ctx, "could not open %s for writing", path);
        return RC_ERR_IO;
    }
    const int k = ctx->k;
    const size_t n = codes.size();
    const unsigned T = rc_host_threads(n, 0);
    const size_t CH = 1u << 20;  // entries formatted per round and thread
    std::vector<std::vector<char>> out(T);
    bool ok = true;
    for (size_t base = 0; base < n && ok; base += CH * T) {
        std::vector<std::thread> th;
        for (unsigned t = 0; t < T; ++t) {
            const size_t lo = std::min(n, base + (size_t)t * CH), hi = std::min(n, lo + CH);
            out[t].clear();
            if (lo < hi) th.emplace_back(rc_dump_format, codes.data(), counts.data(), lo, hi, k, &out[t]);
        }
        for (auto &x : th) x.join();
        for (unsigned t = 0; t < T && ok; ++t)
            if (!out[t].empty() && fwrite(out[t].data(), 1, out[t].size(), fp) != out[t].size()) ok = false;
    }
    if (fclose(fp) != 0) ok = false;
    if (!ok) {
        rc_set_error(ctx, "short write on %s", path);
        return RC_ERR_IO;
    }
    if (n_written) *n_written = (int64_t)n;
    return RC_OK;
}

int rc_table_lookup(rc_ctx *ctx, const uint64_t *codes, size_t n, int32_t *out)
{
    if (!ctx || (n && (!codes || !out))) return RC_ERR_ARG;
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "lookup: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    if (n == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    rc_dev_tmp b_codes, b_out;
    RC_CHECK_HIP(ctx, b_codes.alloc(n * 8));
    RC_CHECK_HIP(ctx, b_out.alloc(n * 4));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(b_codes.p, codes, n * 8, hipMemcpyHostToDevice, ctx->stream));
    int rc = rc_launch_lookup(ctx, b_codes.as<uint64_t>(), n, b_out.as<int32_t>());
    if (rc) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(out, b_out.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

int rc_table_export(rc_ctx *ctx, uint64_t *codes, int32_t *counts, size_t cap, size_t *n_out)
{
    if (!ctx || !n_out || (cap && (!codes || !counts))) return RC_ERR_ARG;
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "export: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    rc_dev_tmp b_codes, b_counts, b_n;
    unsigned long long n = 0;
    RC_CHECK_HIP(ctx, b_codes.alloc((cap + 1) * 8));
    RC_CHECK_HIP(ctx, b_counts.alloc((cap + 1) * 4));
    RC_CHECK_HIP(ctx, b_n.alloc(8));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_n.p, 0, 8, ctx->stream));
    int rc = rc_launch_export(ctx, b_codes.as<uint64_t>(), b_counts.as<int32_t>(), b_n.as<unsigned long long>(), cap);
    if (rc) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(&n, b_n.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    const size_t m = n < cap ? (size_t)n : cap;
    if (m) {
        RC_CHECK_HIP(ctx, hipMemcpy(codes, b_codes.p, m * 8, hipMemcpyDeviceToHost));
        RC_CHECK_HIP(ctx, hipMemcpy(counts, b_counts.p, m * 4, hipMemcpyDeviceToHost));
    }
    *n_out = (size_t)n;
    return RC_OK;
}

int rc_table_digest(rc_ctx *ctx, uint64_t *digest)
{
    if (!ctx || !digest) return RC_ERR_ARG;
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "digest: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    rc_dev_tmp b;
    unsigned long long v = 0;
    RC_CHECK_HIP(ctx, b.alloc(8));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b.p, 0, 8, ctx->stream));
    int rc = rc_launch_digest(ctx, b.as<unsigned long long>());
    if (rc) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(&v, b.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *digest = v;
    return RC_OK;
}

#define RC_SPEC_MAX_BIN (1u << 28)

int rc_table_count_spectrum(rc_ctx *ctx, uint32_t max_bin)
{
    if (!ctx) return RC_ERR_ARG;
    if (max_bin > RC_SPEC_MAX_BIN) {
        rc_set_error(ctx, "count_spectrum: max_bin %u is above %u", max_bin, RC_SPEC_MAX_BIN);
        return RC_ERR_ARG;
    }
    ctx->spec_arm = max_bin;
    return RC_OK;
}

int rc_table_spectrum(rc_ctx *ctx, int source, uint64_t *freq, uint32_t max_bin, rc_spectrum_stats *stats)
{
    if (!ctx) return RC_ERR_ARG;
    if (!freq || max_bin < 1 || max_bin > RC_SPEC_MAX_BIN || (source != 0 && source != 1)) {
        rc_set_error(ctx, "spectrum: source must be 0 (table) or 1 (counted), max_bin 1..%u, freq not NULL", RC_SPEC_MAX_BIN);
        return RC_ERR_ARG;
    }
    uint64_t st[4] = {0, 0, 0, 0};
    if (source == 1) {
        const std::vector<uint64_t> &S = ctx->spec_counted;
        if (S.empty()) {
            rc_set_error(ctx, "spectrum: no counted spectrum (rc_table_count_spectrum before rc_table_count_finish)");
            return RC_ERR_STATE;
        }
        const size_t bound = S.size() - 5;
        if (max_bin > bound) {
            rc_set_error(ctx, "spectrum: max_bin %u is above the bound the count was armed with (%zu)", max_bin, bound);
            return RC_ERR_ARG;
        }
        std::copy(S.begin(), S.begin() + max_bin, freq);
        uint64_t last = 0;  // (counts >= max_bin: the higher bins folded into the last one)
        for (size_t c = max_bin; c <= bound; ++c) last += S[c];
        freq[max_bin] = last;
        std::copy(S.begin() + bound + 1, S.end(), st);
    } else {
        if (!ctx->d_buckets) {
            rc_set_error(ctx, "spectrum: no k-mer table loaded");
            return RC_ERR_STATE;
        }
        RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
        const int rc = rc_table_spectrum_scan(ctx, max_bin, freq, st);
        if (rc) return rc;
    }
    freq[0] = 0;
    if (stats) {
        stats->distinct = st[0];
        stats->total = st[1];
        stats->unique = st[2];
        stats->max_count = st[3];
    }
    return RC_OK;
}

// ---- recount session (include/rcorrector_amd.h) ------------------------------------------------------------------------------
int rc_recount_begin(rc_ctx *ctx, uint32_t max_bin)
{
    if (!ctx) return RC_ERR_ARG;
    if (max_bin < 1 || max_bin > RC_SPEC_MAX_BIN) {
        rc_set_error(ctx, "recount_begin: max_bin must be 1..%u", RC_SPEC_MAX_BIN);
        return RC_ERR_ARG;
    }
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "recount_begin: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    if (ctx->cnt_active) {
        rc_set_error(ctx, "recount_begin: a counting session is open (rc_table_count_finish or rc_table_count_park it first)");
        return RC_ERR_STATE;
    }
    if (ctx->rec_active) {
        rc_set_error(ctx, "recount_begin: a recount session is open already (rc_recount_finish it first)");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_recount_begin_session(ctx, max_bin);
}

static int recount_open(rc_ctx *ctx, const char *what)
{
    if (!ctx->rec_active) {
        rc_set_error(ctx, "%s: call rc_recount_begin first", what);
        return RC_ERR_STATE;
    }
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "%s: no k-mer table loaded", what);
        return RC_ERR_STATE;
    }
    return RC_OK;
}

int rc_recount_add(rc_ctx *ctx, const char *seq, size_t nbytes)
{
    if (!ctx || (nbytes && !seq)) return RC_ERR_ARG;
    if (const int rc = recount_open(ctx, "recount_add")) return rc;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_recount_append(ctx, reinterpret_cast<const uint8_t *>(seq), nbytes, false, ctx->stream);
}

int rc_recount_add_device(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes)
{
    if (!ctx || (nbytes && !d_seq)) return RC_ERR_ARG;
    if (const int rc = recount_open(ctx, "recount_add_device")) return rc;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    return rc_recount_append(ctx, d_seq, nbytes, true, ctx->stream);
}

int rc_recount_follow(rc_ctx *ctx, int on)
{
    if (!ctx) return RC_ERR_ARG;
    ctx->rec_follow = on != 0;
    return RC_OK;
}

int rc_recount_take(rc_ctx *ctx, const void *d_seq, size_t nbytes)
{
    rc_ctx *home = rc_home(ctx);
    if (!home->rec_active || !home->rec_follow || !nbytes) return RC_OK;
    const int rc = rc_recount_append(home, static_cast<const uint8_t *>(d_seq), nbytes, true, ctx->stream);
    if (rc && home != ctx) rc_lane_error(ctx, home);  // (the wait reports through the lane)
    return rc;
}

int rc_recount_finish(rc_ctx *ctx, uint64_t *freq, rc_recount_stats *stats)
{
    if (!ctx) return RC_ERR_ARG;
    if (const int rc = recount_open(ctx, "recount_finish")) {
        if (ctx->rec_active) rc_recount_release(ctx);  // (the table went away under the session)
        return rc;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    if (!freq) {
        rc_recount_release(ctx);
        rc_set_error(ctx, "recount_finish: freq is NULL");
        return RC_ERR_ARG;
    }
    const uint32_t max_bin = ctx->rec_bin;
    std::vector<uint64_t> out;
    const int rc = rc_recount_finish_session(ctx, &out);
    if (rc) return rc;
    std::copy(out.begin(), out.begin() + max_bin + 1, freq);
    freq[0] = 0;
    if (stats) {
        const uint64_t *st = out.data() + max_bin + 1;
        stats->all.distinct = st[0];
        stats->all.total = st[1];
        stats->all.unique = st[2];
        stats->all.max_count = st[3];
        stats->absent_distinct = st[4];
        stats->absent_total = st[5];
    }
    return RC_OK;
}

int rc_table_layout(const rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    if (!ctx->d_buckets) return RC_ERR_STATE;
    return ctx->layout;
}

int rc_table_stats(const rc_ctx *ctx, uint64_t *bytes, uint64_t *buckets, uint64_t *entries)
{
    if (!ctx) return RC_ERR_ARG;
    if (bytes) *bytes = ctx->table_bytes;
    if (buckets) *buckets = ctx->nb_alloc;
    if (entries) *entries = ctx->n_entries;
    return RC_OK;
}

// ---- run parameters --------------------------------------------------------------------------
static int cmp_double(const void *a, const void *b)
{
    double d = *(const double *)a - *(const double *)b;  // CompDouble, main.cpp:39-48
    return d > 0 ? 1 : (d < 0 ? -1 : 0);
}

// main.cpp:310-358
int rc_estimate_error_rate(rc_ctx *c, double wk, double *rate_out)
{
    if (!c || !rate_out) return RC_ERR_ARG;
    rc_ctx_full *ctx = static_cast<rc_ctx_full *>(c);
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "estimate_error_rate: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    // The scan keeps an entry when the largest count among its four last-base variants reaches 1000 and stops after
    // 100 000 of them (main.cpp:329-347): the probes, the test and the selection run on the device over the whole dump
    // (k_error_rate_candidates), the first 100 000 kept entries in dump order come back -- a few hundred KB instead of
    // 16 bytes per entry of the dump each way.
    const int rate_size = 100000;
    std::vector<uint64_t> vals;
    if (!ctx->dump.valid) {
        // no dump file was read (the table was counted here or handed over as arrays): the entries in the order
        // rc_table_write_jfdump would write them -- what the reference would see if it were given that dump
        uint64_t *d_codes = nullptr;
        size_t n = 0;
        int rc = RC_OK;
        if (ctx->counted_codes && ctx->counted_n == (size_t)ctx->n_entries) {  // the table was counted here: its codes are still there
            d_codes = (uint64_t *)ctx->counted_codes;
            n = ctx->counted_n;
            ctx->counted_codes = nullptr;
            ctx->counted_n = 0;
        } else {
            rc = rc_table_codes_device(ctx, &d_codes, &n);
        }
        if (rc) return rc;
        rc = rc_error_rate_candidates(ctx, d_codes, n, true, (size_t)rate_size, &vals);
        (void)hipFree(d_codes);
        if (rc) return rc;
    } else {
        const rc_dump_cache &D = ctx->dump;
        const size_t n = rc_dump_scan_length(D);
        if (n) {
            rc_dev_tmp b_codes;
            RC_CHECK_HIP(ctx, b_codes.alloc(n * 8));
            size_t at = 0;
            for (const auto &ch : D.codes) {
                if (at >= n) break;
                const size_t take = std::min(ch.size(), n - at);
                if (take) RC_CHECK_HIP(ctx, hipMemcpyAsync(b_codes.as<uint64_t>() + at, ch.data(), take * 8, hipMemcpyHostToDevice, ctx->stream));
                at += take;
            }
            int rc = rc_error_rate_candidates(ctx, b_codes.as<uint64_t>(), n, false, (size_t)rate_size, &vals);
            if (rc) return rc;
        }
    }
    std::vector<double> store((size_t)rate_size + 2, 0.0);
    double *r = store.data() + 1;  // r[-1] readable, as in the reference when k == 0
    int cnt = 0;
    for (size_t i = 0; i < vals.size() && cnt < rate_size; ++i) {
        const int mx = (int)(uint32_t)(vals[i] >> 32), second = (int)(uint32_t)vals[i];
        r[cnt++] = (double)second / (double)mx;
    }
    qsort(r, (size_t)cnt, sizeof(double), cmp_double);
    r[cnt] = r[cnt - 1];
    double rate = r[(int)(cnt * wk)];
    if (rate == 0 || cnt < 100) rate = 0.01;
    *rate_out = rate;
    return RC_OK;
}

char rc_bad_quality_from_hist(const int32_t first_hist[300], const int32_t last_hist[300], int32_t total)
{
    int i, cnt = 0, t1, t2;  // main.cpp:108-127
    for (i = 0; i < 300; ++i) {
        cnt += first_hist[i];
        if (cnt > total * 0.05) break;
    }
    t1 = i - 1;
    cnt = 0;
    for (i = 0; i < 300; ++i) {
        cnt += last_hist[i];
        if (cnt > total * 0.05) break;
    }
    t2 = i;
    return (char)(t2 < t1 ? t2 : t1);
}

int rc_set_run_params(rc_ctx *ctx, double error_rate, char bad_quality)
{
    if (!ctx) return RC_ERR_ARG;
    // the codes a counted table was built from wait for rc_estimate_error_rate (which takes them); a caller that sets the
    // parameters itself does not need them: 8 bytes per entry of HBM back (rcorrector_amd.h: rc_table_count_finish)
    if (ctx->counted_codes) {
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        (void)hipFree(ctx->counted_codes);
        ctx->counted_codes = nullptr;
        ctx->counted_n = 0;
    }
    ctx->P.error_rate = error_rate;
    ctx->P.bad_qual = (int)(signed char)bad_quality;
    // the first integer steps of GetBound at this rate (rc_common.h), computed here with the host's -- the
    // reference's -- arithmetic; they travel to the correction kernel with its arguments
    std::vector<uint32_t> steps_v(RC_BOUND_STEPS);
    uint32_t *steps = steps_v.data();
    rc_bound_steps_build(error_rate, steps);
    for (int v = 0; v < RC_BS_INLINE; ++v) ctx->P.bs[v] = steps[v];
    // ... and the whole table stays in device memory for the thresholds beyond those.  A batch in flight, here or in a slot
    // lane, may still read the old one: drained before the buffer can be reallocated or overwritten
    int rc = rc_drain(ctx);
    if (rc) return rc;
    const size_t steps_bytes = (size_t)RC_BOUND_STEPS * sizeof(uint32_t);
    if ((rc = rc_dbuf_reserve(ctx, &ctx->bs_dev, steps_bytes + RC_BOUND_SMALL))) return rc;
    // ... and behind it the bound itself for small counts (rc_run_params::bound_small), again the host's arithmetic
    uint8_t small[RC_BOUND_SMALL];
    for (int c = 0; c < RC_BOUND_SMALL; ++c) {
        const int v = rc_bound_i(c, error_rate);
        small[c] = v >= 0 && v < 255 ? (uint8_t)v : (uint8_t)255;
    }
    RC_CHECK_HIP(ctx, hipMemcpy(ctx->bs_dev.p, steps, steps_bytes, hipMemcpyHostToDevice));
    RC_CHECK_HIP(ctx, hipMemcpy((char *)ctx->bs_dev.p + steps_bytes, small, RC_BOUND_SMALL, hipMemcpyHostToDevice));
    ctx->P.bs_ext = getenv("RC_NO_BS_EXT") ? nullptr : (const uint32_t *)ctx->bs_dev.p;
    ctx->P.bound_small = getenv("RC_NO_BS_EXT") ? nullptr : (const uint8_t *)ctx->bs_dev.p + steps_bytes;
    ctx->P.flags = ctx->env_no_alt ? RC_PF_NO_ALT : 0;
    ctx->params_set = true;
    return RC_OK;
}

int rc_set_quality_bits(rc_ctx *ctx, int on)
{
    if (!ctx) return RC_ERR_ARG;
    ctx->qual_bits = on != 0;
    return RC_OK;
}

void rc_pack_quality_bits(const char *qual, size_t nbytes, char bad_quality, uint8_t *bits)
{
    const signed char bq = (signed char)bad_quality;
    size_t p = 0;
    for (; p + 8 <= nbytes; p += 8) {
        unsigned v = 0;
        for (int j = 0; j < 8; ++j) v |= (unsigned)((signed char)qual[p + j] > bq) << j;
        bits[p >> 3] = (uint8_t)v;
    }
    if (p < nbytes) {
        unsigned v = 0;
        for (int j = 0; p + j < nbytes; ++j) v |= (unsigned)((signed char)qual[p + j] > bq) << j;
        bits[p >> 3] = (uint8_t)v;
    }
}

}  // extern "C"
