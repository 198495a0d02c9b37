// rc_api.hip -- the C ABI of librcorrector_amd.so (include/rcorrector_amd.h): context, table
// load, run-parameter estimation and the batch entry points.  Host code only drives HIP; every
// per-read computation happens in the kernels of rc_table.hip / rc_correct.hip.  There is no CPU
// fallback anywhere in this library.
#include "rc_api_internal.h"
#include <mutex>

static thread_local char g_create_err[512];

void rc_set_error(rc_ctx *ctx, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(ctx ? ctx->err : g_create_err, 512, fmt, ap);
    va_end(ap);
}

int rc_dbuf_reserve(rc_ctx *ctx, rc_dbuf *b, size_t bytes)
{
    if (bytes <= b->bytes) return RC_OK;
    if (b->p) {
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        (void)hipFree(b->p);
        b->p = nullptr;
        b->bytes = 0;
    }
    size_t want = bytes + bytes / 8 + 256;
    RC_CHECK_HIP(ctx, hipMalloc(&b->p, want));
    b->bytes = want;
    return RC_OK;
}

void rc_table_release(rc_ctx *ctx)
{
    // a slot lane may still be probing the table it borrowed (streams of its own): wait for it and take the loan back before
    // the buckets go -- the next batch of that slot gets the new table with its refresh (rc_slot_lane)
    if (ctx->d_buckets && !ctx->buckets_borrowed) {
        (void)rc_drain(ctx);
        for (rc_ctx *ln : ctx->lane) {
            if (!ln || ln->d_buckets != ctx->d_buckets) continue;
            ln->d_buckets = nullptr;
            ln->buckets_borrowed = false;
            ln->n_entries = 0;
        }
    }
    if (ctx->d_buckets && !ctx->buckets_borrowed) (void)hipFree(reinterpret_cast<char *>(ctx->d_buckets) - RC_TABLE_PREFIX_BYTES);
    rc_table_desc &t = ctx->table();  // (the geometry of the table that went stays readable: rc_table_stats)
    t.d_buckets = nullptr;
    t.filter_words = 0;
    t.table_bytes = 0;
    t.n_entries = 0;
    ctx->buckets_borrowed = false;
    if (ctx->counted_codes) (void)hipFree(ctx->counted_codes);
    ctx->counted_codes = nullptr;
    ctx->counted_n = 0;
}

int rc_drain(rc_ctx *ctx)
{
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    // (a batch's follower stream is joined into `stream` before the batch's last kernel: stream2 has something of its own only
    // after a call that failed between fork and join)
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream2));
    rc_timer_resolve(ctx);
    for (rc_ctx *ln : ctx->lane) {
        if (!ln) continue;
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ln->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ln->stream2));
    }
    return RC_OK;
}

int rc_copy_across(rc_ctx *ctx, void *dst, int dst_dev, const void *src, int src_dev, size_t n, hipStream_t st, const char *what)
{
    if (n == 0) return RC_OK;
    if (!getenv("RC_REPLICATE_STAGED")) {  // (tests set it: the path of GPUs without peer access)
        if (dst_dev == src_dev) {
            RC_CHECK_HIP(ctx, hipMemcpyAsync(dst, src, n, hipMemcpyDeviceToDevice, st));
            return RC_OK;
        }
        int can = 0;
        if (hipDeviceCanAccessPeer(&can, dst_dev, src_dev) != hipSuccess) can = 0;
        if (can) {
            const hipError_t e = hipDeviceEnablePeerAccess(src_dev, 0);  // (dst_dev is the current device)
            if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) can = 0;
            (void)hipGetLastError();
        }
        if (can) {
            RC_CHECK_HIP(ctx, hipMemcpyPeerAsync(dst, dst_dev, src, src_dev, n, st));
            return RC_OK;
        }
    }
    // no direct path between the two GPUs: through page-locked host memory, two pieces in flight
    const size_t CH = (size_t)64 << 20;
    const int nbuf = n > CH ? 2 : 1;
    char *h[2] = {nullptr, nullptr};
    hipEvent_t up[2] = {nullptr, nullptr};
    hipError_t e = hipSuccess;
    for (int i = 0; i < nbuf && e == hipSuccess; ++i) {
        e = hipHostMalloc((void **)&h[i], std::min(CH, n), hipHostMallocPortable);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&up[i], hipEventDisableTiming);
    }
    size_t piece = 0;
    for (size_t at = 0; at < n && e == hipSuccess; at += CH, ++piece) {
        const size_t m = std::min(CH, n - at);
        const int b = (int)(piece & 1);
        if (piece >= 2) e = hipEventSynchronize(up[b]);  // the upload that last used this buffer
        if (e == hipSuccess) e = hipSetDevice(src_dev);
        if (e == hipSuccess) e = hipMemcpy(h[b], (const char *)src + at, m, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipSetDevice(dst_dev);
        if (e == hipSuccess) e = hipMemcpyAsync((char *)dst + at, h[b], m, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipEventRecord(up[b], st);
    }
    (void)hipSetDevice(dst_dev);
    const hipError_t arrived = hipStreamSynchronize(st);  // (the buffers go, and the caller may count on the bytes)
    if (e == hipSuccess) e = arrived;
    for (int i = 0; i < 2; ++i) {
        if (h[i]) (void)hipHostFree(h[i]);
        if (up[i]) (void)hipEventDestroy(up[i]);
    }
    if (e != hipSuccess) {
        rc_set_error(ctx, "%s failed: %s", what, hipGetErrorString(e));
        return RC_ERR_HIP;
    }
    return RC_OK;
}

rc_table_view rc_view(const rc_ctx *ctx)
{
    const rc_table_desc &t = ctx->table();
    rc_table_view v;
    v.buckets = t.d_buckets;
    v.nb_home = t.nb_home;
    v.nbuckets_alloc = t.nb_alloc;
    v.layout = t.layout;
    v.ext = t.ext;
    v.k = ctx->k;
    v.filter_words = t.filter_words;
    v.filter = t.filter_words ? t.d_buckets + t.table_bytes / 4 : nullptr;
    v.filter_kind = t.filter_kind;
    v.filter_all = t.filter_all;
    return v;
}

void rc_timer_begin(rc_ctx *ctx)
{
    if (!ctx->profile) return;
    if (ctx->timer_anon >= 0)  // (a launcher that starts its timer twice)
        ctx->timers.rebegin(ctx->timer_anon, ctx->stream);
    else
        ctx->timer_anon = ctx->timers.begin(ctx->stream);
}

void rc_timer_end(rc_ctx *ctx, int which)
{
    if (ctx->timer_anon >= 0) ctx->timers.end(ctx->timer_anon, which, ctx->stream);
    ctx->timer_anon = -1;
}

void rc_timer_begin_on(rc_ctx *ctx, int which, hipStream_t st, bool first)
{
    if (!ctx->profile || !first) return;
    if (ctx->timer_open[which] >= 0)  // (a call that failed between its first and its last chunk left it open)
        ctx->timers.rebegin(ctx->timer_open[which], st);
    else
        ctx->timer_open[which] = ctx->timers.begin(st);
}

void rc_timer_end_on(rc_ctx *ctx, int which, hipStream_t st, bool last)
{
    if (!last) return;
    if (ctx->timer_open[which] >= 0) ctx->timers.end(ctx->timer_open[which], which, st);
    ctx->timer_open[which] = -1;
}

void rc_timer_resolve(rc_ctx *ctx)
{
    ctx->timers.resolve();
}

void rc_lane_error(rc_ctx *ctx, const rc_ctx *lane)
{
    if (ctx != lane) snprintf(ctx->err, sizeof ctx->err, "%s", lane->err);
}

extern "C" {

rc_ctx *rc_slot_lane(rc_ctx *ctx, int slot, bool create, bool refresh)
{
    if (slot <= 0 || slot >= RC_MAX_SLOTS || ctx->is_lane) return ctx;
    if (!create) return ctx->slot_home[slot] ? ctx->slot_home[slot] : ctx;  // a wait: where that slot's batch went
    if (!ctx->env_slot_lanes) {
        ctx->slot_home[slot] = ctx;
        return ctx;
    }
    rc_ctx *&ln = ctx->lane[slot];
    if (!ln) {
        // lanes only overlap when their streams land on different hardware queues: say so, once, if the runtime has few
        static std::once_flag warned;
        std::call_once(warned, [] {
            const char *q = getenv("GPU_MAX_HW_QUEUES");
            if ((!q || atoi(q) < 8) && !getenv("RC_QUIET"))
                fprintf(stderr, "[rcorrector_amd] note: batches in slots > 0 run in lanes with streams of their own, but GPU_MAX_HW_QUEUES is %s: the HIP "
                                "runtime will put them on 4 hardware queues and some will run one after the other. Export GPU_MAX_HW_QUEUES=16 (or call "
                                "rc_runtime_prepare) before the process first touches HIP, or switch the lanes off (rc_set_slot_lanes / RC_SLOT_LANES=0).\n",
                        q ? q : "not set");
        });
        rc_config cfg = {ctx->device, ctx->k, ctx->P.max_fix_per_k};
        char err[256];
        ln = rc_create(&cfg, err, sizeof err);
        if (!ln) {
            rc_set_error(ctx, "slot %d: %s", slot, err);
            return nullptr;
        }
        ln->is_lane = true;
        ln->lane_parent = ctx;
    }
    if (refresh) {  // plain assignments: the table (borrowed, as rc_table_share lends it), the parameters, the mode, the kept arenas
        ln->table() = ctx->table();
        ln->buckets_borrowed = true;
        ln->P = ctx->P;
        ln->params_set = ctx->params_set;
        ln->qual_bits = ctx->qual_bits;
        ln->kept.arenas = ctx->kept.arenas;  // (descriptors only: the chunks stay the parent's)
        ln->profile = ctx->profile;          // measurement follows the batch into its lane (rc_profile_get adds the lanes up)
        ln->phase_prof = ctx->phase_prof;
        ln->phase_prof_print = ctx->phase_prof_print;
        ln->rounds_out = ctx->rounds_out;
    }
    ctx->slot_home[slot] = ln;
    return ln;
}

int rc_runtime_prepare(int hw_queues)
{
    if (hw_queues < 1) return -1;
    if (getenv("GPU_MAX_HW_QUEUES")) return 0;
    char v[16];
    snprintf(v, sizeof v, "%d", hw_queues);
    return setenv("GPU_MAX_HW_QUEUES", v, 0) == 0 ? 1 : -1;
}

rc_ctx *rc_create(const rc_config *cfg, char *errbuf, size_t errbuf_len)
{
    auto fail = [&](const char *msg) -> rc_ctx * {
        if (errbuf && errbuf_len) snprintf(errbuf, errbuf_len, "%s", msg);
        return nullptr;
    };
    if (!cfg) return fail("rc_create: null config");
    // (Slot lanes want their streams on hardware queues of their own -- GPU_MAX_HW_QUEUES, the host's to export before HIP
    // starts: rc_runtime_prepare / rcorrector_amd.h.  The library does not touch its host's environment from here.)
    if (cfg->k < 1 || cfg->k > 32) return fail("rc_create: k must be in 1..32 (run_rcorrector.pl:225-228)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail("rc_create: no HIP device available (this library has no CPU fallback)");
    if (cfg->device < 0 || cfg->device >= ndev) return fail("rc_create: device ordinal out of range");
    if (hipSetDevice(cfg->device) != hipSuccess) return fail("rc_create: hipSetDevice failed");
    rc_ctx_full *ctx = new (std::nothrow) rc_ctx_full();
    if (!ctx) return fail("rc_create: out of memory");
    ctx->err[0] = 0;
    ctx->device = cfg->device;
    ctx->k = cfg->k;
    ctx->P.k = cfg->k;
    ctx->P.max_fix_per_k = cfg->max_fix_per_k > 0 ? cfg->max_fix_per_k : 4;
    ctx->P.error_rate = 0.01;
    ctx->P.bad_qual = 0;
    memset(ctx->P.bs, 0, sizeof ctx->P.bs);
    ctx->P.bs_ext = nullptr;
    ctx->P.bound_small = nullptr;
    ctx->P.flags = 0;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess) ctx->n_cu = prop.multiProcessorCount;
    for (int &t : ctx->timer_open) t = -1;
    bool made = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) == hipSuccess &&
                hipStreamCreateWithFlags(&ctx->stream2, hipStreamNonBlocking) == hipSuccess &&
                hipEventCreateWithFlags(&ctx->pipe_join, hipEventDisableTiming) == hipSuccess;
    for (hipEvent_t &e : ctx->pipe_ev) made = made && hipEventCreateWithFlags(&e, hipEventDisableTiming) == hipSuccess;
    if (!made || hipMalloc(&ctx->work.p, RC_WORK_BYTES) != hipSuccess) {
        delete ctx;
        return fail("rc_create: could not create stream/events");
    }
    ctx->work.bytes = RC_WORK_BYTES;
    (void)hipMemset(ctx->work.p, 0, RC_WORK_BYTES);
    if (const char *e = getenv("RC_PHASE_PROF")) ctx->phase_prof = ctx->phase_prof_print = atoi(e) != 0;
    if (const char *e = getenv("RC_TABLE_LOAD")) {
        ctx->table_load = ctx->table_load_packed = atof(e);
        ctx->table_load_set = true;
    }  // tuning knob
    if (const char *e = getenv("RC_TABLE_LAYOUT")) ctx->layout_pref = strcmp(e, "wide") != 0;         // dev: A/B the slot layouts
    ctx->env_k2_wave_per_read = getenv("RC_K2_WAVE_PER_READ") != nullptr;  // dev: force the wave-per-read threshold kernel
    ctx->env_no_classify = getenv("RC_NO_CLASSIFY") != nullptr;            // dev: every read goes through k_correct
    ctx->env_timing = getenv("RC_TIMING") != nullptr;
    ctx->env_no_fuse = getenv("RC_NO_FUSE") != nullptr;
    if (const char *dd = getenv("RC_FUSED_DEDUP")) ctx->env_dedup = atoi(dd) != 0 ? 1 : 0;
    if (const char *xo = getenv("RC_FUSED_XCD")) ctx->env_fused_xcd = atoi(xo) != 0;
    if (const char *qd = getenv("RC_PROBE_QUAD")) ctx->env_quad = atoi(qd) != 0 ? 1 : 0;
    if (const char *kl = getenv("RC_K3_LOCAL")) ctx->env_k3_local = atoi(kl) != 0;
    if (const char *pc = getenv("RC_PIPELINE_CHUNKS")) ctx->env_pipe_chunks = atoi(pc) > 0 ? atoi(pc) : 0;
    if (const char *pg = getenv("RC_PIPELINE_GRID_DIV")) ctx->env_pipe_grid_div = atoi(pg) > 0 ? atoi(pg) : 0;
    if (const char *wt = getenv("RC_FUSED_WAVE_TILES")) ctx->env_wave_tiles = atoi(wt) != 0;
    ctx->env_no_tier = getenv("RC_NO_TIER") != nullptr;
    if (const char *e = getenv("RC_FORCE_EC")) {
        const int v = atoi(e);
        if (v == 9 || v == 10) ctx->env_force_ec = v;
    }
    ctx->env_k3_generic = getenv("RC_K3_GENERIC") != nullptr;
    ctx->env_no_single = getenv("RC_NO_SINGLE") != nullptr;
    ctx->env_no_alt = getenv("RC_NO_ALT") != nullptr;  // dev / tests: no alternative chains in the search's speculation rounds
    if (const char *e = getenv("RC_LOCALITY")) ctx->locality_mode = !strcmp(e, "force") ? 1 : (!strcmp(e, "off") ? -1 : 0);  // tests / A-B
    if (const char *e = getenv("RC_K3_GRID_WAVES")) ctx->env_k3_grid_waves = atoi(e);
    if (const char *e = getenv("RC_SLOT_LANES")) ctx->env_slot_lanes = atoi(e) != 0;
    return ctx;
}

void rc_destroy(rc_ctx *c)
{
    if (!c) return;
    rc_ctx_full *ctx = static_cast<rc_ctx_full *>(c);
    for (rc_ctx *&ln : ctx->lane) {  // (they borrow this context's table and arenas: they go first)
        if (ln) {
            ln->kept.arenas.clear();
            rc_destroy(ln);
        }
        ln = nullptr;
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->stream2) (void)hipStreamSynchronize(ctx->stream2);
    rc_dbuf *bufs[] = {&ctx->counts, &ctx->strong, &ctx->info, &ctx->stack, &ctx->work,
                       &ctx->h_seq, &ctx->h_qual, &ctx->h_off, &ctx->h_res, &ctx->trace, &ctx->cls, &ctx->worklist, &ctx->sel_tmp,
                       &ctx->loc_a, &ctx->loc_list, &ctx->loc_span, &ctx->tier_flag, &ctx->tier_list, &ctx->cand, &ctx->single_list, &ctx->runs, &ctx->bs_dev, &ctx->weak_planes, &ctx->trust_planes, &ctx->trust_part};
    for (rc_dbuf *b : bufs)
        if (b->p) (void)hipFree(b->p);
    if (ctx->slots) {
        for (int i = 0; i < RC_MAX_SLOTS; ++i) {
            rc_slot &sl = ctx->slots[i];
            if (sl.e_done) (void)hipEventSynchronize(sl.e_done);
            rc_hbuf *hb[] = {&sl.p_seq, &sl.p_qual, &sl.p_off, &sl.p_res, &sl.p_in, &sl.p_fix, &sl.p_nfix};
            for (rc_hbuf *h : hb)
                if (h->p) (void)hipHostFree(h->p);
            rc_dbuf *db[] = {&sl.d_seq, &sl.d_qual, &sl.d_off, &sl.d_res, &sl.d_packed, &sl.d_exc, &sl.d_fix};
            for (rc_dbuf *d : db)
                if (d->p) (void)hipFree(d->p);
            for (rc_slot_payload &pl : sl.payload) {
                if (pl.p.p) (void)hipHostFree(pl.p.p);
                if (pl.d.p) (void)hipFree(pl.d.p);
            }
            hipEvent_t ev[] = {sl.e_h2d, sl.e_k, sl.e_done};
            for (hipEvent_t e : ev)
                if (e) (void)hipEventDestroy(e);
        }
    }
    rc_observed_drop_all(ctx, RC_OBS_ALL, true);  // (what the batch observers staged, here and in the slots; the lanes are gone)
    delete[] ctx->slots;
    if (ctx->s_h2d) (void)hipStreamDestroy(ctx->s_h2d);
    if (ctx->s_d2h) (void)hipStreamDestroy(ctx->s_d2h);
    ctx->cnt.release();
    ctx->kept.release();
    rc_recount_release(ctx);
    rc_report_release(ctx);
    for (void *acc : ctx->dup_acc)  // (the duplicate census's keys; its scratch went with the buffers above)
        if (acc) (void)hipFree(acc);
    if (ctx->trust_acc) (void)hipFree(ctx->trust_acc);  // (the trust profile's counts; its scratch went with the buffers above)
    if (ctx->ovl_acc) (void)hipFree(ctx->ovl_acc);      // (the mate-overlap report's counts)
    rc_recur_release(ctx);                               // (the recurrence census's keys)
    rc_table_release(ctx);
    ctx->timers.release();
    for (hipEvent_t e : ctx->pipe_ev)
        if (e) (void)hipEventDestroy(e);
    if (ctx->pipe_join) (void)hipEventDestroy(ctx->pipe_join);
    if (ctx->stream2) (void)hipStreamDestroy(ctx->stream2);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

const char *rc_last_error(const rc_ctx *ctx) { return ctx ? ctx->err : g_create_err; }

int rc_set_slot_lanes(rc_ctx *ctx, int on)
{
    if (!ctx) return RC_ERR_ARG;
    ctx->env_slot_lanes = on != 0;
    return RC_OK;
}

int rc_device_numa_node(const rc_ctx *ctx)
{
    if (!ctx) return -1;
    char bus[64];
    if (hipDeviceGetPCIBusId(bus, (int)sizeof bus, ctx->device) != hipSuccess) return -1;
    for (char *p = bus; *p; ++p)
        if (*p >= 'A' && *p <= 'F') *p = (char)(*p - 'A' + 'a');  // sysfs spells the address in lower case
    char path[160];
    snprintf(path, sizeof path, "/sys/bus/pci/devices/%s/numa_node", bus);
    FILE *fp = fopen(path, "r");
    if (!fp) return -1;
    int node = -1;
    if (fscanf(fp, "%d", &node) != 1) node = -1;
    fclose(fp);
    return node;
}

int rc_device_memory(rc_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes)
{
    if (!ctx) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    size_t f = 0, t = 0;
    RC_CHECK_HIP(ctx, hipMemGetInfo(&f, &t));
    if (free_bytes) *free_bytes = (uint64_t)f;
    if (total_bytes) *total_bytes = (uint64_t)t;
    return RC_OK;
}

// ---- measurement -----------------------------------------------------------------------------
int rc_profile_enable(rc_ctx *ctx, int on)
{
    if (!ctx) return RC_ERR_ARG;
    ctx->profile = on != 0;
    if (!ctx->phase_prof_print) ctx->phase_prof = on == 2;
    for (rc_ctx *ln : ctx->lane) {  // (and a lane that exists already; new ones copy the flags when they take a batch)
        if (!ln) continue;
        ln->profile = ctx->profile;
        ln->phase_prof = ctx->phase_prof;
    }
    return RC_OK;
}

int rc_profile_get(rc_ctx *ctx, int kernel, double *total_ms, uint64_t *launches)
{
    if (!ctx || kernel < 0 || kernel >= RC_T_COUNT) return RC_ERR_ARG;
    // the pairs still pending are waited for here (no kernel is waited for when it is launched: rc_timer_pool.h)
    (void)hipSetDevice(ctx->device);
    rc_timer_resolve(ctx);
    double ms = ctx->timers.total[kernel].ms;
    uint64_t n = ctx->timers.total[kernel].launches;
    for (rc_ctx *ln : ctx->lane) {  // (the batches of slots > 0 ran in lane contexts)
        if (!ln) continue;
        rc_timer_resolve(ln);
        ms += ln->timers.total[kernel].ms;
        n += ln->timers.total[kernel].launches;
    }
    if (total_ms) *total_ms = ms;
    if (launches) *launches = n;
    return RC_OK;
}

int rc_profile_reset(rc_ctx *ctx)
{
    if (!ctx) return RC_ERR_ARG;
    ctx->timers.reset();
    for (int &t : ctx->timer_open) t = -1;
    ctx->timer_anon = -1;
    ctx->k3_listed = ctx->k3_rounds = ctx->k3_requests = 0;
    for (rc_ctx *ln : ctx->lane) {
        if (!ln) continue;
        ln->timers.reset();
        for (int &t : ln->timer_open) t = -1;
        ln->timer_anon = -1;
        ln->k3_listed = ln->k3_rounds = ln->k3_requests = 0;
    }
    return RC_OK;
}

int rc_profile_correct_counters(rc_ctx *ctx, uint64_t *reads_listed, uint64_t *gather_rounds, uint64_t *bucket_requests)
{
    if (!ctx) return RC_ERR_ARG;
    uint64_t a = ctx->k3_listed, b = ctx->k3_rounds, c = ctx->k3_requests;
    for (rc_ctx *ln : ctx->lane) {
        if (!ln) continue;
        a += ln->k3_listed;
        b += ln->k3_rounds;
        c += ln->k3_requests;
    }
    if (reads_listed) *reads_listed = a;
    if (gather_rounds) *gather_rounds = b;
    if (bucket_requests) *bucket_requests = c;
    return RC_OK;
}

int rc_profile_read_rounds(rc_ctx *ctx, int32_t *d_rounds)
{
    if (!ctx) return RC_ERR_ARG;
    ctx->rounds_out = d_rounds;
    for (rc_ctx *ln : ctx->lane)
        if (ln) ln->rounds_out = d_rounds;
    return RC_OK;
}

int rc_selftest_get_bound(rc_ctx *ctx, const int32_t *c, size_t n, double error_rate, int32_t *out_int, double *out_dbl)
{
    if (!ctx || (n && (!c || !out_int || !out_dbl))) return RC_ERR_ARG;
    if (n == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    rc_dev_tmp b_c, b_i, b_d;
    RC_CHECK_HIP(ctx, b_c.alloc(n * 4));
    RC_CHECK_HIP(ctx, b_i.alloc(n * 4));
    RC_CHECK_HIP(ctx, b_d.alloc(n * 8));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(b_c.p, c, n * 4, hipMemcpyHostToDevice, ctx->stream));
    int rc = rc_launch_selftest_bound(ctx, b_c.as<int32_t>(), n, error_rate, b_i.as<int32_t>(), b_d.as<double>());
    if (rc) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(out_int, b_i.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(out_dbl, b_d.p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

}  // extern "C"

// test support: the fix list of a launch into device arrays of cap + RC_SELFTEST_FIX_SLACK entries that held the canary, and what
// came of it into the caller's arrays (the count, the arrays with their slack).  `launch` gets d_n_fix, d_fix_pos, d_fix_chr.
template <class Launch>
static int selftest_fix_list(rc_ctx *ctx, uint32_t cap, uint32_t *n_fix_out, uint32_t *fix_pos_out, uint8_t *fix_chr_out, Launch launch)
{
    const size_t room = (size_t)cap + RC_SELFTEST_FIX_SLACK;
    rc_dev_tmp b_n, b_pos, b_chr;
    RC_CHECK_HIP(ctx, b_n.alloc(64));
    RC_CHECK_HIP(ctx, b_pos.alloc(room * 4));
    RC_CHECK_HIP(ctx, b_chr.alloc(room));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_pos.p, RC_SELFTEST_CANARY, room * 4, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_chr.p, RC_SELFTEST_CANARY, room, ctx->stream));
    if (const int rc = launch(b_n.as<uint32_t>(), b_pos.as<uint32_t>(), b_chr.as<uint8_t>())) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    RC_CHECK_HIP(ctx, hipMemcpyAsync(n_fix_out, b_n.p, 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(fix_pos_out, b_pos.p, room * 4, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(fix_chr_out, b_chr.p, room, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

extern "C" {

// test support: the packed boundary's device side alone (rc_transport.hip through its production launchers) -- no table, no run
// parameters, no correction: `after` stands for the arena the correction kernels would have left.
int rc_selftest_transport_packed(rc_ctx *ctx, const uint32_t *packed, size_t nbytes, const uint32_t *off, uint32_t n_reads, const uint32_t *exc_pos,
                                 const uint8_t *exc_chr, uint32_t n_exc, const uint8_t *after, uint8_t *unpacked_out, uint32_t *n_fix_out, uint32_t cap,
                                 uint32_t *fix_pos_out, uint8_t *fix_chr_out)
{
    if (!ctx || !unpacked_out || !n_fix_out || !fix_pos_out || !fix_chr_out || nbytes >= (1ull << 32) || (size_t)cap + RC_SELFTEST_FIX_SLACK >= (1ull << 32) ||
        (nbytes && (!packed || !after)) || (n_reads && !off) || (n_exc && (!exc_pos || !exc_chr)))
        return RC_ERR_ARG;
    // (the terminator and exception kernels write seq[off[i+1]-1] and seq[exc_pos[i]] unchecked: what rc_submit_packed refuses)
    if (n_reads && (off[0] != 0 || off[n_reads] != nbytes)) return RC_ERR_ARG;
    for (uint32_t i = 0; i < n_reads; ++i)
        if (off[i + 1] <= off[i]) return RC_ERR_ARG;
    for (uint32_t i = 0; i < n_exc; ++i)
        if (exc_pos[i] >= nbytes) return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t n_words = (nbytes + 15) / 16, arena = n_words * 16 + RC_SELFTEST_ARENA_SLACK;  // (d_seq of submit_packed)
    rc_dev_tmp b_packed, b_seq, b_off, b_epos, b_echr;
    RC_CHECK_HIP(ctx, b_packed.alloc(n_words * 4 + 64));
    RC_CHECK_HIP(ctx, b_seq.alloc(arena));
    RC_CHECK_HIP(ctx, b_off.alloc(((size_t)n_reads + 1) * 4));
    RC_CHECK_HIP(ctx, b_epos.alloc((size_t)n_exc * 4));
    RC_CHECK_HIP(ctx, b_echr.alloc(n_exc));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_seq.p, RC_SELFTEST_CANARY, arena, ctx->stream));
    if (n_words) RC_CHECK_HIP(ctx, hipMemcpyAsync(b_packed.p, packed, n_words * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_reads) RC_CHECK_HIP(ctx, hipMemcpyAsync(b_off.p, off, ((size_t)n_reads + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
    if (n_exc) {
        RC_CHECK_HIP(ctx, hipMemcpyAsync(b_epos.p, exc_pos, (size_t)n_exc * 4, hipMemcpyHostToDevice, ctx->stream));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(b_echr.p, exc_chr, n_exc, hipMemcpyHostToDevice, ctx->stream));
    }
    int rc = rc_launch_unpack(ctx, b_packed.as<uint32_t>(), nbytes, b_off.as<uint32_t>(), n_reads, b_epos.as<uint32_t>(), b_echr.as<uint8_t>(), n_exc,
                              b_seq.as<uint8_t>());
    if (rc) {
        (void)hipStreamSynchronize(ctx->stream);
        return rc;
    }
    RC_CHECK_HIP(ctx, hipMemcpyAsync(unpacked_out, b_seq.p, arena, hipMemcpyDeviceToHost, ctx->stream));
    // the corrected bytes; the padding behind them stays as the unpack left it
    if (nbytes) RC_CHECK_HIP(ctx, hipMemcpyAsync(b_seq.p, after, nbytes, hipMemcpyHostToDevice, ctx->stream));
    rc = selftest_fix_list(ctx, cap, n_fix_out, fix_pos_out, fix_chr_out, [&](uint32_t *d_n, uint32_t *d_pos, uint8_t *d_chr) {
        return rc_launch_fix_list(ctx, b_packed.as<uint32_t>(), nbytes, b_seq.as<uint8_t>(), b_epos.as<uint32_t>(), n_exc, d_n, cap, d_pos, d_chr);
    });
    (void)hipStreamSynchronize(ctx->stream);  // (the uploads read the caller's arrays until here, whatever became of the launches)
    return rc;
}

// test support: k_fix_list_bytes alone, the uncorrected bytes at any alignment (the ranges of kept arenas a resident batch names)
int rc_selftest_transport_bytes(rc_ctx *ctx, const uint8_t *orig_a, size_t na, uint32_t shift_a, const uint8_t *orig_b, size_t nb, uint32_t shift_b,
                                const uint8_t *after, uint32_t *n_fix_out, uint32_t cap, uint32_t *fix_pos_out, uint8_t *fix_chr_out)
{
    if (!ctx || !n_fix_out || !fix_pos_out || !fix_chr_out || shift_a > 15 || shift_b > 15 || na >= (1ull << 32) || nb >= (1ull << 32) ||
        na + nb >= (1ull << 32) || (size_t)cap + RC_SELFTEST_FIX_SLACK >= (1ull << 32) || (na && !orig_a) || (nb && !orig_b) || (na + nb && !after))
        return RC_ERR_ARG;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nbytes = na + nb, arena = ((nbytes + 15) & ~(size_t)15) + RC_SELFTEST_ARENA_SLACK;  // (d_seq of submit_resident)
    const size_t span_a = shift_a + na + RC_SELFTEST_ARENA_SLACK, span_b = shift_b + nb + RC_SELFTEST_ARENA_SLACK;
    rc_dev_tmp b_a, b_b, b_seq;
    RC_CHECK_HIP(ctx, b_a.alloc(span_a + 16));  // (hipMalloc aligns to 256 bytes; whole 16-byte words behind the slack)
    RC_CHECK_HIP(ctx, b_b.alloc(span_b + 16));
    RC_CHECK_HIP(ctx, b_seq.alloc(arena));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_seq.p, RC_SELFTEST_CANARY, arena, ctx->stream));
    if (orig_a) RC_CHECK_HIP(ctx, hipMemcpyAsync(b_a.p, orig_a, span_a, hipMemcpyHostToDevice, ctx->stream));
    if (orig_b) RC_CHECK_HIP(ctx, hipMemcpyAsync(b_b.p, orig_b, span_b, hipMemcpyHostToDevice, ctx->stream));
    if (nbytes) RC_CHECK_HIP(ctx, hipMemcpyAsync(b_seq.p, after, nbytes, hipMemcpyHostToDevice, ctx->stream));
    const int rc = selftest_fix_list(ctx, cap, n_fix_out, fix_pos_out, fix_chr_out, [&](uint32_t *d_n, uint32_t *d_pos, uint8_t *d_chr) {
        return rc_launch_fix_list_bytes(ctx, b_a.as<uint8_t>() + shift_a, na, nb ? b_b.as<uint8_t>() + shift_b : nullptr, nb, b_seq.as<uint8_t>(), d_n, cap,
                                        d_pos, d_chr);
    });
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

// test support: which kernel finished each read of the batch this context ran last -- cls (0: finished before k_correct; k_single
// clears it, rc_single.h), cand (the threshold kernel's flag for k_single: the number of stretches) and runs (the stretches, x in
// the low word) as they lie in HBM.  Copies only: no kernel is launched, and the correction kernels know nothing of it.
// (rc_correct_batch is slot 0, which runs in the context itself -- rc_slot_lane -- so these are the buffers it wrote.)
int rc_debug_routes(rc_ctx *ctx, uint8_t *cls_out, uint8_t *cand_out, uint64_t *runs_out, uint32_t n)
{
    if (!ctx || !cls_out || !cand_out || !runs_out) return RC_ERR_ARG;
    const char *why = nullptr;
    if (ctx->routes_state == rc_ctx::RC_ROUTES_NONE)
        why = "no batch has run in this context";
    else if (ctx->routes_state == rc_ctx::RC_ROUTES_FAILED)
        why = "the last batch did not run to its end";
    else if (ctx->routes_state == rc_ctx::RC_ROUTES_TIERED)
        why = "the last batch ran in length tiers (a read of more than 160 bases): the arrays are rewritten per pass";
    else if (!ctx->cls_ready)
        why = "the last batch ran without classification (cls_ready is false)";
    else if (!ctx->cand_ready)
        why = "the last batch ran without k_single's candidates (cand_ready is false)";
    if (why) {
        rc_set_error(ctx, "debug_routes: %s", why);
        return RC_ERR_STATE;
    }
    if (n != ctx->routes_n) {
        rc_set_error(ctx, "debug_routes: n = %u, the last batch had %u reads", n, ctx->routes_n);
        return RC_ERR_STATE;
    }
    if (n == 0) return RC_OK;
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpy(cls_out, ctx->cls.p, n, hipMemcpyDeviceToHost));
    RC_CHECK_HIP(ctx, hipMemcpy(cand_out, ctx->cand.p, n, hipMemcpyDeviceToHost));
    RC_CHECK_HIP(ctx, hipMemcpy(runs_out, ctx->runs.p, (size_t)n * 8, hipMemcpyDeviceToHost));
    return RC_OK;
}

// test support: how many batches this context and its slot lanes ran as a chunked pipeline (rc_correct_pipelined with *ran = true)
// and how many non-empty chunks those launched.  Host integers: no device memory is read, no stream is touched.
int rc_debug_pipeline(rc_ctx *ctx, uint64_t *batches, uint64_t *chunks)
{
    if (!ctx) return RC_ERR_ARG;
    uint64_t b = ctx->pipe_batches, c = ctx->pipe_chunks;
    for (const rc_ctx *ln : ctx->lane) {  // (the batches its slot lanes ran, as rc_summary adds them)
        if (!ln) continue;
        b += ln->pipe_batches;
        c += ln->pipe_chunks;
    }
    if (batches) *batches = b;
    if (chunks) *chunks = c;
    return RC_OK;
}

int rc_summary(const rc_ctx *c, uint64_t *total_reads, uint64_t *total_corrections)
{
    if (!c) return RC_ERR_ARG;
    rc_ctx *ctx = const_cast<rc_ctx *>(c);  // (reads device memory; the counters themselves do not change)
    unsigned long long v[2] = {0, 0};
    RC_CHECK_HIP(ctx, hipSetDevice(ctx->device));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpy(v, (char *)ctx->work.p + RC_WORK_SUMMARY_OFF, sizeof v, hipMemcpyDeviceToHost));
    for (rc_ctx *ln : ctx->lane) {  // (the batches its slot lanes ran)
        if (!ln) continue;
        unsigned long long w[2] = {0, 0};
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ln->stream));
        RC_CHECK_HIP(ctx, hipMemcpy(w, (char *)ln->work.p + RC_WORK_SUMMARY_OFF, sizeof w, hipMemcpyDeviceToHost));
        v[0] += w[0];
        v[1] += w[1];
    }
    if (total_reads) *total_reads = v[0];
    if (total_corrections) *total_corrections = v[1];
    return RC_OK;
}

}  // extern "C"
