// rc_internal.h -- context object and cross-TU declarations of librcorrector_amd.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <atomic>
#include <mutex>
#include <type_traits>
#include <utility>
#include <vector>

#include "rc_correct_core.h"
#include "rc_timer_pool.h"

#define RC_CHECK_HIP(ctx, expr)                                                                  \
    do {                                                                                         \
        hipError_t _e = (expr);                                                                  \
        if (_e != hipSuccess) {                                                                  \
            rc_set_error((ctx), "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, \
                         __LINE__);                                                              \
            return RC_ERR_HIP;                                                                   \
        }                                                                                        \
    } while (0)

// scoped device allocation: freed on every exit path of the function that owns it
struct rc_dev_tmp {
    void *p = nullptr;
    rc_dev_tmp() = default;
    rc_dev_tmp(const rc_dev_tmp &) = delete;
    rc_dev_tmp &operator=(const rc_dev_tmp &) = delete;
    ~rc_dev_tmp() { reset(); }
    void reset()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
    }
    hipError_t alloc(size_t bytes)
    {
        reset();
        return hipMalloc(&p, bytes ? bytes : 1);
    }
    template <class T>
    T *as() const { return static_cast<T *>(p); }
};

// grow-only device buffer
struct rc_dbuf {
    void *p = nullptr;
    size_t bytes = 0;
};

// the reads of a counting session in HBM: the arenas handed over, views into a few large allocations (chunks: a hipMalloc /
// hipFree per arena -- dozens per run, each a round trip through the kernel driver -- cost more than counting them on a busy host)
struct rc_ctx;
struct rc_arena_set {
    std::vector<rc_dbuf> arenas, chunks;
    size_t chunk_used = 0;  // bytes of the last chunk handed out
    size_t total = 0;       // bytes of reads
    void release();
    // a copy of an arena (device or host memory) into the set, on stream st; complete on return.  Errors go to ctx, as `what`
    int keep(rc_ctx *ctx, const uint8_t *seq, size_t nbytes, bool from_device, hipStream_t st, const char *what);
    void move_to(rc_arena_set &to)  // `to` holds what this set held, this set nothing
    {
        to.release();
        std::swap(*this, to);
    }
};

#define RC_MAX_SLOTS 4

// the per-read payloads a batch of the slot transports can carry, 16 bytes per read each, in the order their kernels are
// launched and their values come down: the weak-k-mer profile, the k-mer depth, the hit profile against a second k-mer set
enum rc_payload_kind { RC_PAY_WEAK, RC_PAY_DEPTH, RC_PAY_SCREEN, RC_PAY_COUNT };

// trust profile: the counts of one batch in flight, an rc_trust_counts of its bases as they arrived and one of its bases as
// corrected, until the batch completes (staged == false: none were taken); gen: the profile they were taken for
struct rc_trust_staged {
    rc_dbuf buf;
    bool staged = false;
    uint64_t gen = 0;
    uint32_t n_reads = 0;
    int mode = 0, max_read_len = 0;
    int32_t min_count = 1;
};

// mate-overlap report: the counts of one batch in flight, an rc_mate_overlap in HBM, until the batch completes (staged == false:
// none were taken); gen: the session they were taken for
struct rc_overlap_staged {
    rc_dbuf buf;
    bool staged = false;
    uint64_t gen = 0;
};

// What the batch observers (rc_api_observe.hip) keep for one batch in flight, from the submit that staged it to the completion
// that accepts it: the duplicate census's keys (dup_units before | dup_units after; 0: none were taken) and the census they
// were taken for, the trust profile's counts, the mate-overlap report's counts, and the correction report's counts where they
// are staged (rep_staged: this batch left some), and the recurrence census's site keys (recur_staged: this batch was looked at;
// recur_n keys in recur_keys, of recur_changes changes, recur_contexted of them contexted) and the census they were taken for.
// One per slot, and one per context for the entry points that have no slot.
enum { RC_OBS_DUPS = 1, RC_OBS_TRUST = 2, RC_OBS_REPORT = 4, RC_OBS_OVERLAP = 8, RC_OBS_RECUR = 16, RC_OBS_ALL = 31 };
struct rc_batch_observed {
    rc_dbuf dup_keys;
    size_t dup_units = 0;
    uint64_t dup_gen = 0;
    rc_trust_staged trust;
    rc_overlap_staged ovl;
    rc_dbuf rep;
    bool rep_staged = false;
    rc_dbuf recur_keys, recur_counts;
    bool recur_staged = false;
    uint64_t recur_n = 0, recur_changes = 0, recur_contexted = 0, recur_gen = 0;
    // nothing staged any more for these observers; free_bufs: their buffers go too
    void drop(int parts, bool free_bufs);
    void reset() { drop(RC_OBS_ALL, false); }
};

// the timer pool's back end (rc_timer_pool.h): HIP's events
struct rc_hip_events {
    typedef hipEvent_t event;
    typedef hipStream_t stream;
    bool create(event *e) { return hipEventCreate(e) == hipSuccess; }
    void destroy(event e) { (void)hipEventDestroy(e); }
    void record(event e, stream st) { (void)hipEventRecord(e, st); }
    void wait(event e) { (void)hipEventSynchronize(e); }
    bool elapsed(event a, event b, float *ms) { return hipEventElapsedTime(ms, a, b) == hipSuccess; }
};

enum { RC_T_PROBE = 0, RC_T_THRESH = 1, RC_T_CORRECT = 2, RC_T_SINGLE = 3, RC_T_WEAK = 4, RC_T_TRUST_PLANES = 5, RC_T_TRUST = 6, RC_T_DEPTH = 7, RC_T_SCREEN = 8, RC_T_NORM = 9, RC_T_COUNT };

// what describes a k-mer table in HBM: a context that shares or copies another's table, or a slot lane its parent's, takes all of it
// in one assignment, and rc_view reads nothing else (but k)
struct rc_table_desc {
    uint32_t *d_buckets = nullptr;
    uint32_t nb_home = 0;
    int layout = 0;       // slot layout of the table (rc_common.h): 0 WIDE, 1 PACKED
    int ext = 0;          // PACKED: remainder bits kept above the count (rc_table_view::ext)
    uint32_t nb_alloc = 0;
    size_t n_entries = 0;   // accepted entries (duplicates included)
    size_t table_bytes = 0;
    uint32_t filter_words = 0;  // absence filter behind the bucket array (rc_common.h: rc_table_view::filter), 0 = none
    int filter_kind = 0;        // rc_table_view::filter_kind of the filter that is there
    int filter_all = 0;         // rc_table_view::filter_all
    rc_table_desc &table() { return *this; }
    const rc_table_desc &table() const { return *this; }
};

struct rc_ctx : rc_table_desc {
    int device = 0;
    int k = 23;
    int n_cu = 256;
    hipStream_t stream = nullptr;
    // Chunked pipeline (rc_correct_device_impl): the follower stream -- the compactions, k_single and k_correct of a chunk of the
    // locality list run there while the fused probe + threshold kernel of the next chunks runs on `stream` -- a ring of events
    // for the forks (chunk c's fused kernel is done) and the event of the join (`stream` waits for it before k_summary, so whoever
    // orders work behind `stream`, or waits for it, has the follower's work too).  Created with the context.
    hipStream_t stream2 = nullptr;
    enum { RC_PIPE_EVENTS = 8 };
    hipEvent_t pipe_ev[RC_PIPE_EVENTS] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}, pipe_join = nullptr;
    uint32_t pipe_ev_next = 0;
    int env_pipe_chunks = -1;    // RC_PIPELINE_CHUNKS=<C>: 0 / 1 = off, C >= 2 = that many chunks at any batch size; -1: the default (RC_PIPE_*)
    int env_pipe_grid_div = 0;   // RC_PIPELINE_GRID_DIV=<d> (dev / A-B): the follower kernels' grids divided by d under the pipeline; 0: the default
    uint64_t pipe_batches = 0, pipe_chunks = 0;  // rc_debug_pipeline (test support): batches this context ran as a pipeline, non-empty chunks it launched
    bool profile = false;
    bool phase_prof = false;  // the instrumented build of k_correct runs (RC_PHASE_PROF=1 or rc_profile_enable(ctx, 2))
    bool phase_prof_print = false;  // ... and prints its per-phase cycle accounting (RC_PHASE_PROF=1, dev aid)
    uint64_t k3_listed = 0, k3_rounds = 0, k3_requests = 0;  // accumulated by the instrumented build
    int32_t *rounds_out = nullptr;  // rc_profile_read_rounds: where the instrumented build leaves every read's gather rounds
    // kernel timers: event pairs recorded now, waited for and added up later (rc_timer_resolve).  timer_open[kind] = the pair of
    // that kind whose end is still to come (-1: none); timer_anon = rc_timer_begin's
    rc_timer_pool<rc_hip_events, RC_T_COUNT> timers;
    int timer_open[RC_T_COUNT];
    int timer_anon = -1;

    rc_run_params P;
    bool params_set = false;
    bool qual_bits = false;  // quality arenas are bit arrays (rc_set_quality_bits)
    // Slot lanes: slot s > 0 of the asynchronous entry points runs in a context of its own (lane[s], created at its first use:
    // own streams, events and scratch; the table, the run parameters and the kept arenas are this context's, lent), so that
    // the kernels of batches in different slots overlap on the GPU -- a batch's last waves on its slowest reads under the
    // next batch's probe kernel.  RC_SLOT_LANES=0: every slot in this context, one compute stream (round 4's behaviour).
    rc_ctx *lane[4] = {nullptr, nullptr, nullptr, nullptr};
    rc_ctx *slot_home[4] = {nullptr, nullptr, nullptr, nullptr};  // where the batch a slot holds was submitted (lanes can be switched)
    bool is_lane = false;
    bool env_slot_lanes = true;

    // k-mer table in HBM: its description is the base rc_table_desc
    bool buckets_borrowed = false;  // rc_table_share: another context owns d_buckets
    double table_load = 0.50;  // target slot load factor of the next build (WIDE layout)
    bool table_load_set = false;  // RC_TABLE_LOAD given: no size-dependent choice
    double table_load_packed = 0.50;  // ... (PACKED layout)
    int layout_pref = 1;  // 0: always WIDE (RC_TABLE_LAYOUT=wide)
    // the canonical codes of the entries a table was counted from (rc_count_finish), kept until the ERROR_RATE pass has used them
    // or the table goes: that pass wants every entry's code, and reading them back out of the buckets (k_export: a decode and
    // a probe walk per slot) costs more than the 8 bytes per entry it frees
    void *counted_codes = nullptr;
    size_t counted_n = 0;

    // -verbose support: iterations recorded per read by k_correct (0 = off) and the record buffer
    int trace_cap = 0;
    rc_dbuf trace;

    // k-mer counter (rc_table_count_begin/add/finish): the arenas handed over so far, kept in HBM until finish
    rc_arena_set cnt;
    bool cnt_active = false;
    // rc_table_count_keep(on): finish() leaves the arenas here instead of releasing them -- the reads of a data set
    // that was counted on this GPU are corrected where they lie (rc_submit_resident)
    bool cnt_keep = false;
    rc_arena_set kept;
    // k-mer count spectrum of the counter (rc_table_count_spectrum): the bound finish() bins to (0 = off), and what the last
    // finish (on ctxs[0] of a sharded one) saw -- freq[bound + 1], then distinct, total, unique, max_count; empty: none
    // since the last count_begin
    uint32_t spec_arm = 0;
    std::vector<uint64_t> spec_counted;
    // recount session (rc_recount_begin): a second counting session that builds no table -- its arenas in chunks of its own
    // (the counter's and the kept arenas are never touched), the bound its spectrum is binned to, and whether the batches
    // that complete on this context (its slot lanes included: rc_home) append their corrected arena (rc_recount_follow)
    rc_arena_set rec;
    bool rec_active = false, rec_follow = false;
    uint32_t rec_bin = 0;
    std::mutex rec_mutex;
    rc_ctx *lane_parent = nullptr;  // a slot lane: the context whose slots it serves
    // correction report (rc_change_report_begin): the accumulator, RC_REPORT_WORDS 64-bit counts laid out as rc_change_report
    // (nullptr: not armed; the batches of this context's slot lanes add to it too: rc_home).  In the context a batch RUNS
    // in (a lane included): the copy of its arena taken before the first correction kernel (grow-only), on that context's one
    // compute stream
    unsigned long long *rep_acc = nullptr;
    rc_dbuf rep_snap;
    // weak-k-mer profile (rc_weak_profile_device / rc_weak_profile_into; kernels in rc_weak.hip).  weak_planes: the two bit planes
    // of the arena profiled last, scratch of the context the kernels run in (they serialise on its compute stream)
    rc_dbuf weak_planes;
    // The per-read payloads' one-shot registrations (rc_api_payload.hip: rc_weak_profile_into, rc_read_depth_into,
    // rc_read_screen_into; kernels in rc_weak.hip, rc_depth.hip, rc_screen.hip).  payload_reg[kind][slot]: per slot of THIS
    // context's entry points, where the next batch submitted there leaves its reads' 16 bytes each (out == nullptr: nowhere) --
    // the submit takes it and hands it to the context the batch runs in (a lane included) as payload_cur[kind], which the
    // slot's download step consumes
    struct rc_payload_reg {
        void *out = nullptr;             // rc_read_weak / rc_read_depth / rc_read_screen[total]
        int32_t min_count = 1;           // weak, screen
        const rc_ctx *screen = nullptr;  // screen: the context whose table the batch's reads are looked up in -- the caller keeps it
                                         // and its table alive until the batch's wait
    };
    rc_payload_reg payload_reg[RC_PAY_COUNT][RC_MAX_SLOTS], payload_cur[RC_PAY_COUNT];
    // duplicate census (rc_dup_census_begin; kernels in rc_dups.hip).  In the context it was opened on (the batches of its slot
    // lanes add to it too: rc_home): the keys of every unit seen, version 0 = before and 1 = after correction, 16 bytes per
    // unit each, dup_n units of dup_cap; dup_gen counts the begins (keys a batch staged for one census never reach the next).
    // obs_mutex: the lanes' waits append to the census and add to the trust profile concurrently.
    std::atomic<bool> dup_open{false};  // (read by the lanes' submits without the mutex)
    void *dup_acc[2] = {nullptr, nullptr};
    size_t dup_n = 0, dup_cap = 0;
    uint64_t dup_gen = 0;
    std::mutex obs_mutex;
    // trust profile (rc_trust_profile_begin; kernels in rc_trust.hip).  In the context it was opened on (the batches of its slot
    // lanes add to it too: rc_home): trust_acc, two rc_trust_counts in HBM (before | after), the reads seen per mate, the
    // threshold, and trust_gen, which counts the begins; the lanes' waits add under obs_mutex.  In the context a batch or
    // rc_trust_profile_device RUNS in: the bit planes and the wavefronts' partial counts of the arena profiled last (scratch,
    // serialised on its compute stream)
    std::atomic<bool> trust_open{false};  // (read by the lanes' submits without the mutex)
    void *trust_acc = nullptr;
    uint64_t trust_reads[2] = {0, 0};
    int32_t trust_min = 1;
    uint64_t trust_gen = 0;
    rc_dbuf trust_planes, trust_part;
    // mate-overlap report (rc_mate_overlap_begin; kernel in rc_overlap.hip).  In the context it was opened on (the batches of its
    // slot lanes add to it too: rc_home): ovl_acc, an rc_mate_overlap in HBM, the two thresholds, and ovl_gen, which counts the
    // begins; the lanes' waits add under obs_mutex.  The arena as it arrived is rep_snap, the correction report's copy
    std::atomic<bool> ovl_open{false};  // (read by the lanes' submits without the mutex)
    void *ovl_acc = nullptr;
    int32_t ovl_min = 30, ovl_pct = 10;
    uint64_t ovl_gen = 0;
    // recurrence census (rc_recur_census_begin; kernels in rc_recur.hip).  In the context it was opened on (the batches of its slot
    // lanes add to it too: rc_home): the site keys of every contexted change seen, 8 bytes each, recur_n of recur_cap, the two
    // totals, and recur_gen, which counts the begins; the lanes' waits append under obs_mutex.  The arena as it arrived is
    // rep_snap, the correction report's copy
    std::atomic<bool> recur_open{false};  // (read by the lanes' submits without the mutex)
    void *recur_acc = nullptr;
    size_t recur_n = 0, recur_cap = 0;
    uint64_t recur_changes = 0, recur_contexted = 0, recur_gen = 0;
    // in the context a batch RUNS in: what the observers staged for the batch of an entry point that has no slot
    // (rc_correct_device, rc_correct_batch_traced)
    rc_batch_observed obs;

    // batch scratch
    rc_dbuf counts;   // int32 per arena byte
    rc_dbuf strong;   // int32 per read
    rc_dbuf info;     // int32 per read
    bool thr_ready = false;  // strong / info hold this batch's thresholds (the threshold kernel ran)
    rc_dbuf cls;      // uint8 per read: 1 = still needs k_correct (written by the threshold kernel)
    rc_dbuf cand;     // uint8 per read: 1 = candidate of k_single (written by the threshold kernel with cls)
    rc_dbuf single_list;  // the candidates' read indices, ascending (compaction of cand)
    rc_dbuf runs;     // uint2 per read, candidates only: their untrusted stretches (rc_kernel_args::runs)
    rc_dbuf bs_dev;   // RC_BOUND_STEPS uint32: the inverse of GetBound at the run's ERROR_RATE (rc_run_params::bs_ext)
    bool cand_ready = false;
    rc_dbuf worklist; // RC_WORK_CLASSES sections of work_stride uint32 each: the reads with cls == 4, 3, 2, 1, ascending within a section
    rc_dbuf sel_tmp;  // rocPRIM scratch of the compaction
    rc_dbuf loc_a, loc_list, loc_span;  // locality order of a batch (rc_launch_locality_order): the reads, and where each lies in the arena
    rc_dbuf tier_flag, tier_list;  // mixed-length batches: the reads of the middle / long tier in locality order (rc_launch_tier_lists)
    size_t tier_stride = 0;        // uint32 entries between the two sections of tier_list
    bool env_fused_xcd = false;  // RC_FUSED_XCD=1 (dev): the fused probe kernel's tiles in XCD-contiguous order
    bool env_wave_tiles = false;  // RC_FUSED_WAVE_TILES=1 (dev): the fused probe kernel with one wavefront (four reads) per workgroup
    bool env_k3_local = false;  // RC_K3_LOCAL=1 (dev): k_correct's work list in the batch's locality order (non-tiered batches)
    int env_quad = -1;   // RC_PROBE_QUAD=0 / 1 (dev / tests): bucket reads by the lane / by the quad (rc_table_lookup_quad); -1: the default
    int env_dedup = -1;  // RC_FUSED_DEDUP=0 / 1 (dev / tests): the fused probe kernel without / with its per-tile k-mer set; -1: the table decides (rc_launch_probe_threshold_list)
    bool env_no_fuse = false;  // RC_NO_FUSE=1 (dev): separate probe and threshold kernels in locality order too
    int env_force_ec = 0;      // RC_FORCE_EC=9|10 (dev / tests): at least this many count registers per lane in the 160-base instances
    bool env_no_tier = false;  // RC_NO_TIER=1 (dev / tests): no length tiers, the longest read of a batch decides every kernel
    bool env_k3_generic = false;  // RC_K3_GENERIC=1 (dev / tests): the any-k instance of k_correct even where a compiled-for-k one exists
    bool env_no_single = false;  // RC_NO_SINGLE=1 (dev / tests): k_single is not launched (rc_launch_single) -- every listed read goes to k_correct; the
                                 // threshold kernel flags its candidates all the same, and rc_debug_routes shows which reads it would have been offered
    bool env_no_alt = false;  // RC_NO_ALT=1 (dev / tests): rc_run_params::flags |= RC_PF_NO_ALT
    int locality_mode = 0;  // 0: large batches over large tables, 1: always (RC_LOCALITY=force), -1: never (RC_LOCALITY=off)
    bool cls_ready = false;  // cls / worklist describe this batch
    // what rc_debug_routes (test support) may say of cls / cand / runs: the batch rc_correct_device_impl ran last in this context
    enum { RC_ROUTES_NONE, RC_ROUTES_FAILED, RC_ROUTES_TIERED, RC_ROUTES_WHOLE } routes_state = RC_ROUTES_NONE;  // (FAILED: also while one runs;
                                                                                                                // TIERED: the arrays are rewritten per pass)
    uint32_t routes_n = 0;  // the batch's reads (RC_ROUTES_WHOLE)
    size_t work_stride = 0;  // uint32 entries between the sections of worklist
    // getenv() results, read once at rc_create
    bool env_k2_wave_per_read = false, env_no_classify = false, env_timing = false;
    int env_k3_grid_waves = 0;  // dev: persistent k_correct waves per SIMD actually launched (0 = as compiled)
    rc_dbuf stack;    // search stack frames
    rc_dbuf work;     // work counters
    rc_dbuf h_seq, h_qual, h_off, h_res;  // device staging for the host-buffer entry point (traced path)

    // asynchronous host-buffer path (rc_submit / rc_wait): copy streams and per-slot staging
    hipStream_t s_h2d = nullptr, s_d2h = nullptr;
    struct rc_slot *slots = nullptr;  // RC_MAX_SLOTS of them, created on first use

    char err[512];
};

void rc_set_error(rc_ctx *ctx, const char *fmt, ...);
int rc_dbuf_reserve(rc_ctx *ctx, rc_dbuf *b, size_t bytes);
rc_table_view rc_view(const rc_ctx *ctx);
// frees the table this context owns (the allocation starts RC_TABLE_PREFIX_BYTES before d_buckets)
void rc_table_release(rc_ctx *ctx);
// the context a slot lane serves, else the context itself: where the accumulators of the batch observers and the recount session live
static inline rc_ctx *rc_home(rc_ctx *ctx) { return ctx->is_lane && ctx->lane_parent ? ctx->lane_parent : ctx; }
// ctx's device current, and what ctx and its slot lanes (streams of their own) have queued has run
int rc_drain(rc_ctx *ctx);
// n bytes from device memory of GPU src_dev to device memory of GPU dst_dev (or the same), queued on `st`, a stream of dst_dev,
// which is the current device: device to device, peer to peer where the GPUs can, else (or with RC_REPLICATE_STAGED set) through
// page-locked host memory in 64 MB pieces, two in flight -- the bytes have then arrived on return, and a failure reads
// "`what` failed: ..."
int rc_copy_across(rc_ctx *ctx, void *dst, int dst_dev, const void *src, int src_dev, size_t n, hipStream_t st, const char *what);
// Kernel timers (profiling on: rc_profile_enable).  Nothing here waits for the GPU: the pairs are resolved by rc_timer_resolve
// -- rc_profile_get, rc_drain, a full pool.  rc_timer_begin / _end: one interval on ctx->stream.  rc_timer_begin_on / _end_on:
// the interval of kind `which` on stream st, begun only if `first` and ended only if `last` -- the chunked pipeline launches a
// kind's kernel once per chunk and times the span from its first launch to its last as ONE launch.
void rc_timer_begin(rc_ctx *ctx);
void rc_timer_end(rc_ctx *ctx, int which);
void rc_timer_begin_on(rc_ctx *ctx, int which, hipStream_t st, bool first);
void rc_timer_end_on(rc_ctx *ctx, int which, hipStream_t st, bool last);
void rc_timer_resolve(rc_ctx *ctx);
// f(std::bool_constant<ext>{}): the launch of a kernel that is compiled for tables with and without remainder-extension bits
// (rc_device.h: EXT), written once -- rc_with_ext(ctx->ext, [&](auto ext) { ... k_probe<decltype(ext)::value> ... });
template <class F>
static inline void rc_with_ext(int ext, F &&f)
{
    if (ext)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// rc_table.hip
int rc_build_table_from_device_pairs(rc_ctx *ctx, const uint64_t *d_canon, const int32_t *d_counts,
                                     size_t n);
int rc_launch_canonicalize(rc_ctx *ctx, uint64_t *d_codes, size_t n);
int rc_launch_lookup(rc_ctx *ctx, const uint64_t *d_codes, size_t n, int32_t *d_out);
int rc_launch_probe(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, int32_t *d_counts);
int rc_launch_selftest_bound(rc_ctx *ctx, const int32_t *d_c, size_t n, double e, int32_t *d_oi, double *d_od);
int rc_launch_export(rc_ctx *ctx, uint64_t *d_codes, int32_t *d_counts, unsigned long long *d_n, size_t cap);
// k-mer count spectrum (rc_device.h: rc_spec_add): the table's into host arrays freq[max_bin + 1], st[4]; one slice's run-length
// counts added to d_out (freq[max_bin + 1], then the four statistics; zeroed by the caller) on stream st
int rc_table_spectrum_scan(rc_ctx *ctx, uint32_t max_bin, uint64_t *freq, uint64_t *st);
int rc_launch_spectrum_counts(rc_ctx *ctx, hipStream_t st, const uint32_t *d_cnt, size_t n, uint32_t max_bin, unsigned long long *d_out);
// one sorted slice of a recount session (distinct codes and their counts) against the table, added to d_out (max_bin + 1 + 6
// uint64: the spectrum's, then absent_distinct, absent_total; zeroed by the caller) on stream st
int rc_launch_census(rc_ctx *ctx, hipStream_t st, const uint64_t *d_uniq, const uint32_t *d_cnt, size_t n, uint32_t max_bin, unsigned long long *d_out);
int rc_table_entries_in_dump_order(rc_ctx *ctx, std::vector<uint64_t> *codes, std::vector<int32_t> *counts);
int rc_error_rate_candidates(rc_ctx *ctx, const uint64_t *d_codes, size_t n, bool by_hash, size_t want, std::vector<uint64_t> *vals);
int rc_table_codes_device(rc_ctx *ctx, uint64_t **d_codes, size_t *n);
int rc_launch_last_base_variants(rc_ctx *ctx, const uint64_t *d_codes, size_t n, int32_t *d_max2);
int rc_launch_digest(rc_ctx *ctx, unsigned long long *d_out);
int rc_launch_locality_order(rc_ctx *ctx, const struct rc_device_batch_args &a, size_t nbytes);
int rc_launch_probe_list(rc_ctx *ctx, const struct rc_device_batch_args &a, size_t nbytes, int32_t *d_counts, int skip_hi = -1);
int rc_launch_tier_lists(rc_ctx *ctx, const struct rc_device_batch_args &a, int s_hi, int m_hi);
// K1 over section `section` (0: middle tier, 1: long tier) of ctx->tier_list; a.max_len = the longest read of that tier
int rc_launch_probe_tier(rc_ctx *ctx, const struct rc_device_batch_args &a, size_t nbytes, int32_t *d_counts, int section);
int rc_launch_compact(rc_ctx *ctx, const uint8_t *d_cls, uint32_t n, uint32_t *d_list, size_t stride, uint32_t *d_count);
int rc_launch_compact_local(rc_ctx *ctx, const uint8_t *d_cls, uint32_t n, uint32_t *d_list, size_t stride, uint32_t *d_count);
int rc_launch_compact_flag(rc_ctx *ctx, const uint8_t *d_flag, uint32_t n, uint32_t *d_list, size_t stride, uint32_t *d_count);
// the two compactions over positions [lo, hi) of the batch's locality order alone (ctx->loc_list), on stream st: the lists
// receive the reads at those positions whose flag says so
int rc_launch_compact_range(rc_ctx *ctx, hipStream_t st, const uint8_t *d_cls, uint32_t lo, uint32_t hi, uint32_t *d_list, size_t stride, uint32_t *d_count);
int rc_launch_compact_flag_range(rc_ctx *ctx, hipStream_t st, const uint8_t *d_flag, uint32_t lo, uint32_t hi, uint32_t *d_list, size_t stride, uint32_t *d_count);

// rc_count.hip
int rc_count_begin(rc_ctx *ctx);
int rc_count_add(rc_ctx *ctx, const uint8_t *seq, size_t nbytes, bool from_device);
int rc_count_finish(rc_ctx *ctx, int min_count, int64_t *n_kmers);
int rc_count_park(rc_ctx *ctx);
int rc_count_finish_sharded(rc_ctx **cs, int n, int min_count, int64_t *n_kmers);
int rc_count_reads(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, int min_count, int64_t *n_kmers);
// recount session: begin / append a copy of an arena (on stream st; complete on return) / the passes and the census kernel
// (out: freq[rec_bin + 1], distinct, total, unique, max_count, absent_distinct, absent_total) / release (also on every error)
int rc_recount_begin_session(rc_ctx *ctx, uint32_t max_bin);
int rc_recount_append(rc_ctx *ctx, const uint8_t *seq, size_t nbytes, bool from_device, hipStream_t st);
int rc_recount_finish_session(rc_ctx *ctx, std::vector<uint64_t> *out);
void rc_recount_release(rc_ctx *ctx);

// rc_correct.hip
#define RC_TIER_ALL 0x7fffffff  // rc_kernel_args::tier_hi: no length tiers
#define RC_Q_MAX_KCNT 256        // the quarter-wave threshold kernel's widest instance (rc_quarter.h): k-mers / bases per read
#define RC_Q_MAX_LEN 320
struct rc_device_batch_args {
    int mode;            // 0 single, 1 paired (reads [0,n/2) are mates of [n/2,n)), 2 interleaved
    uint32_t n;          // reads
    uint8_t *seq;        // arena, reads NUL-terminated
    size_t nbytes = 0;   // bytes of the arena: no kernel reads a byte at or past it
    const uint8_t *qual; // same offsets (or one bit per arena byte, see rc_set_quality_bits)
    int qual_bits = 0;
    uint32_t qual_split = 0xFFFFFFFFu, qual_base2 = 0;
    const uint32_t *off; // n+1
    int32_t *ret, *l, *m, *h;
    int max_len;         // longest read in the batch (bases)
    int tier_lo = -1, tier_hi = RC_TIER_ALL;  // length tier of this pass (rc_kernel_args::tier_lo / tier_hi)
    int pair_override = -1;                   // rc_kernel_args::pair_override
    // the tier's reads as a list in locality order and its length on the device (rc_launch_tier_lists), or nullptr: the
    // threshold kernel of the pass then walks the whole batch and leaves the other tiers' reads out
    const uint32_t *tier_list = nullptr, *tier_n = nullptr;
};
int rc_launch_threshold(rc_ctx *ctx, const rc_device_batch_args &a, bool classify);
// One chunk of the chunked pipeline, as the launchers see it.  The fused kernel takes tiles [tile_lo, tile_hi) of the locality
// list and says which list positions [lo, hi) those are; k_single and k_correct run on stream st over lists made of those
// positions.  first / last: the chunk is the call's first / last (timers, rc_timer_begin_on); grid_div: the persistent
// kernels' grids divided by it.  nullptr everywhere: the whole batch on ctx->stream.
struct rc_chunk {
    hipStream_t st = nullptr;
    uint32_t tile_lo = 0, tile_hi = 0;
    uint32_t lo = 0, hi = 0;
    bool first = true, last = true;
    int grid_div = 1;
};
int rc_launch_correct(rc_ctx *ctx, const rc_device_batch_args &a, const rc_chunk *ch = nullptr);
int rc_launch_single(rc_ctx *ctx, const rc_device_batch_args &a, bool *ran, const rc_chunk *ch = nullptr);
int rc_launch_probe_threshold_list(rc_ctx *ctx, const rc_device_batch_args &a, size_t nbytes, bool *done, rc_chunk *ch = nullptr);
// tiles of the fused kernel over a batch (0: the batch does not fit it) -- what the chunks are cut from
uint32_t rc_fused_tiles(const rc_ctx *ctx, const rc_device_batch_args &a, uint32_t *reads_per_tile);
int rc_launch_summary(rc_ctx *ctx, const int32_t *d_ret, uint32_t n);
int rc_launch_kmer_info(rc_ctx *ctx, const rc_device_batch_args &a);

// rc_report.hip: the correction report.  RC_REPORT_WORDS: 64-bit counts of an rc_change_report (8 per-mate totals, six
// tables of 1024, 20 substitutions, 3 quality classes, 65 per-read bins)
#define RC_REPORT_WORDS (8 + 6 * 1024 + 20 + 3 + 65)
// every read of the batch against d_snap (the arena before correction, at the arena's alignment modulo 16), counted into d_out
int rc_launch_change_report(rc_ctx *ctx, const rc_device_batch_args &a, const uint8_t *d_snap, unsigned long long *d_out);
int rc_launch_report_commit(rc_ctx *ctx, const unsigned long long *d_staged, unsigned long long *d_out);

// rc_weak.hip: solid / weak bit planes of the arena into `planes` (grow-only), then d_out[r] = the rc_read_weak of read r
int rc_launch_weak_profile(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int min_count, rc_dbuf *planes,
                           void *d_out);

// rc_depth.hip: d_out[r] = the rc_read_depth of read r, one launch; a read whose offsets leave the arena, or of more than
// RC_MAX_READ_LENGTH - 1 bases, gets four zeros
int rc_launch_read_depth(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, void *d_out);

// rc_screen.hip: d_out[r] = the rc_read_screen of read r against `screen`'s table (same k, same device: checked), one launch on
// ctx's stream; the reads that are none get four zeros, as above
int rc_launch_read_screen(rc_ctx *ctx, const rc_ctx *screen, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int min_count,
                          void *d_out);

// rc_norm.hip: d_keep[u] = the outcome of unit u (rc_norm.h) from the rc_read_depth of its mates, the outcomes and the unit depths
// added to d_tally (4 + 2 (max_bin + 1) uint64 in HBM); one launch, no table
int rc_launch_norm_select(rc_ctx *ctx, const void *d_depth, uint32_t n_units, int mode, uint64_t unit_base, uint32_t target, uint32_t min_cov, uint64_t seed,
                          uint32_t max_bin, uint8_t *d_keep, uint64_t *d_tally);

// rc_weak.hip: the two bit planes alone (what rc_launch_weak_profile launches first): *solid / *weak point into `planes`,
// *lead = the bytes between the 16-byte boundary the planes start at and d_seq.  rc_trust.hip: the planes of the arena at
// min_count into `planes`, every wavefront's counts into `partials` (both grow-only), their column sums added to d_counts
// (an rc_trust_counts in HBM); max_read_len picks the instance.  rc_launch_trust_add: d_dst[i] += d_src[i], n_words uint64
int rc_launch_weak_planes(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, int min_count, rc_dbuf *planes, const uint64_t **solid_out,
                          const uint64_t **weak_out, uint32_t *lead_out);
int rc_launch_trust_profile(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int max_read_len, int mode,
                            int min_count, rc_dbuf *planes, rc_dbuf *partials, void *d_counts);
int rc_launch_trust_add(rc_ctx *ctx, const void *d_src, void *d_dst, uint32_t n_words);

// rc_overlap.hip: the pairs of two arenas that share d_off (mode 1 or 2, n_reads / 2 pairs), added to d_counts (an rc_mate_overlap
// in HBM); max_read_len picks the instance
int rc_launch_mate_overlap(rc_ctx *ctx, const uint8_t *d_before, const uint8_t *d_after, size_t nbytes, const uint32_t *d_off, uint32_t n_reads,
                           int max_read_len, int mode, int min_overlap, int max_mismatch_pct, void *d_counts);

// rc_trim.hip: d_out[r] = the rc_read_trim of read r (rc_trim.h), d_keep[u] (may be null) = unit u is kept, the counts added to
// d_tally (an rc_trim_tally in HBM, may be null); one launch, no table; max_read_len picks the instance.  params: an rc_trim_params that has been checked
int rc_launch_read_trim(rc_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int max_read_len,
                        int mode, const void *params, void *d_out, uint8_t *d_keep, void *d_tally);

// rc_merge.hip: the pairs of an arena (mode 1 or 2) merged into a new compact arena d_mseq / d_mqual (may be null) / d_moff
// (n_reads / 2 + 1 entries), d_rows[u] = the rc_read_merge of unit u (rc_merge.h), the counts added to d_tally (an rc_merge_tally
// in HBM, may be null); plan kernel, scan, write kernel on ctx's stream, scratch in ctx->sel_tmp; no table.  params: an
// rc_merge_params that has been checked
int rc_launch_read_merge(rc_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int max_read_len,
                         int mode, const void *params, void *d_rows, uint8_t *d_mseq, uint8_t *d_mqual, uint32_t *d_moff, size_t out_cap, void *d_tally);

// rc_dups.hip: one 128-bit key per unit of an arena (mode as rc_device_batch: n_reads units, or n_reads / 2 pairs) on stream st;
// the census of n keys in HBM (left as they are) into host arrays copies[max_bin + 1], *distinct -- synchronous
int rc_launch_read_keys(rc_ctx *ctx, hipStream_t st, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int mode,
                        uint64_t *d_keys);
int rc_dup_census_run(rc_ctx *ctx, const uint64_t *d_keys, size_t n, uint32_t max_bin, uint64_t *copies, uint64_t *distinct);

// rc_recur.hip: the site keys of the contexted changes between two arenas of one alignment modulo 16 that share d_off, appended
// to d_keys (never past cap) on stream st; d_counts[3] (zeroed first) = changes, contexted changes, keys appended -- the third
// passes cap where they did not fit.  The census of n keys in HBM (left as they are) into host arrays -- synchronous
int rc_launch_change_keys(rc_ctx *ctx, hipStream_t st, const uint8_t *d_before, const uint8_t *d_after, const uint32_t *d_off, uint32_t n_reads, size_t nbytes,
                          uint64_t *d_keys, uint64_t cap, uint64_t *d_counts);
int rc_recur_census_run(rc_ctx *ctx, const uint64_t *d_keys, size_t n, uint32_t max_bin, uint32_t min_count, uint32_t max_sites, uint64_t *recur,
                        uint64_t *sites, uint64_t *sites_recurrent, uint64_t *changes_at_recurrent, uint64_t *top_key, uint64_t *top_count, uint32_t *n_top);

// rc_transport.hip: the packed boundary (include/rcorrector_amd.h: rc_packed_batch)
int rc_launch_unpack(rc_ctx *ctx, const uint32_t *d_packed, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, const uint32_t *d_exc_pos,
                     const uint8_t *d_exc_chr, uint32_t n_exc, uint8_t *d_seq);
int rc_launch_fix_list_bytes(rc_ctx *ctx, const uint8_t *d_orig_a, size_t bytes_a, const uint8_t *d_orig_b, size_t bytes_b, const uint8_t *d_seq,
                              uint32_t *d_n_fix, uint32_t cap, uint32_t *d_fix_pos, uint8_t *d_fix_chr);
int rc_launch_fix_list(rc_ctx *ctx, const uint32_t *d_packed, size_t nbytes, const uint8_t *d_seq, const uint32_t *d_exc_pos, uint32_t n_exc,
                       uint32_t *d_n_fix, uint32_t cap, uint32_t *d_fix_pos, uint8_t *d_fix_chr);

// k_correct's work list comes in RC_WORK_CLASSES sections, taken in order: the reads expected to be
// the most expensive first, so that the last waves of a launch are not left alone with them
// (cls value of a read = 1 + its section counted from the back; cls 0 = finished by the threshold kernel)
#define RC_WORK_CLASSES 4
#ifndef RC_FILTER_KIND_DEFAULT
#define RC_FILTER_KIND_DEFAULT 1  // "core": config 4's k_correct 6.31 -> 5.61 s (RC_TABLE_FILTER_KIND=plain for the other)
#endif
// layout of rc_ctx::work (bytes): RC_WORK_CLASSES x RC_HEADS queue heads of k_correct, 128 B apart,
// then the lengths of the work-list sections, then the phase counters of PROF builds
#define RC_WORK_BYTES 5120
#define RC_WORK_NWORK_OFF 4096
#define RC_WORK_NSINGLE_OFF 4160  // 4 x uint32: lengths of the three sections of k_single's list, 0 (it reads them like the four section lengths)
#define RC_WORK_NTIER_OFF 4192    // 2 x uint32: reads of the middle / long length tier (rc_launch_tier_lists)
#define RC_WORK_PHASE_OFF 4224
#define RC_WORK_SUMMARY_OFF 4608  // 2 x uint64: reads, corrected bases (never reset)
