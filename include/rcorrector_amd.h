/*
 * rcorrector_amd.h -- C ABI of librcorrector_amd.so: the MI355X-native drop-in for Rcorrector's
 * per-read correction path (stage 3 of run_rcorrector.pl).
 *
 * Plain pointers and sizes only; no C++/torch types.  Each entry point names the reference
 * interface (/root/reference, v1.0.7) it replaces.  INTEGRATION.md shows the binding a maintainer
 * of the reference would add in main.cpp.
 *
 * Conventions
 *   - every function returns 0 on success or a negative rc_status; rc_last_error() has the text.
 *     The library never calls exit() (the reference exits on I/O errors, File.h:69-73).
 *   - k-mer codes are the reference's KmerCode::GetCode() values (KmerCode.h:39): 2 bits per base,
 *     A0 C1 G2 T3, first base in the most significant position, k <= 32.
 *   - a context owns one GPU, its stream, the k-mer table in HBM and all scratch memory.  One
 *     context per GPU / per host thread; reads shard across contexts with no communication
 *     (the table is replicated), SURVEY.md §8(e).
 *   - there is NO CPU fallback: without a usable HIP device rc_create() fails.
 */
#ifndef RCORRECTOR_AMD_H
#define RCORRECTOR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rc_ctx rc_ctx;

typedef enum {
    RC_STATUS_OK = 0,
    RC_STATUS_ARG = -1,   /* bad argument */
    RC_STATUS_HIP = -2,   /* HIP runtime error */
    RC_STATUS_IO = -3,    /* file could not be read */
    RC_STATUS_STATE = -4, /* call sequence error (no table, no run parameters, ...) */
    RC_STATUS_NOMEM = -5,
    RC_STATUS_NOSPACE = -6 /* rc_wait_packed / rc_wait_resident: more substitutions than fix_cap (n_fix = how many): the batch's
                              ret / l / m / h are complete, its fix list is not -- resubmit with more room, or through rc_submit */
} rc_status;

typedef struct {
    int device;        /* HIP device ordinal */
    int k;             /* kmerLength, main.cpp:133,200-204 (1..32) */
    int max_fix_per_k; /* MAX_FIX_PER_K / -maxcorK, main.cpp:159,215-219 */
} rc_config;

/* replaces: KmerCode kcode(kmerLength); Store kmers;  (main.cpp:140,270) */
rc_ctx *rc_create(const rc_config *cfg, char *errbuf, size_t errbuf_len);
void rc_destroy(rc_ctx *ctx);
const char *rc_last_error(const rc_ctx *ctx);
/* the NUMA node of the host the context's GPU hangs off (its PCI device's numa_node), or -1 if the system does
 * not say: a host that feeds the GPU from page-locked buffers wants its threads and those buffers there
 * (the reference has no counterpart: its workers are plain pthreads, main.cpp:479-483) */
int rc_device_numa_node(const rc_ctx *ctx);
/* free and total bytes of the context's GPU memory right now (hipMemGetInfo): what a host checks before it asks the
 * k-mer counter to keep a data set's bases in HBM (rc_table_count_keep).  No reference counterpart. */
int rc_device_memory(rc_ctx *ctx, uint64_t *free_bytes, uint64_t *total_bytes);

/* ---- k-mer table (Store.h:17-88) ------------------------------------------------------------ */
/* replaces the load loop main.cpp:294-308 when the caller has already parsed the dump:
 * n x Store::Put(code, count) in index order (a later duplicate overrides an earlier one,
 * Store.h:55).  codes may be forward or canonical; counts <= 1 must already be filtered. */
int rc_table_build(rc_ctx *ctx, const uint64_t *codes, const int32_t *counts, size_t n);
/* same with the arrays already in HBM (d_codes is canonicalised in place) */
int rc_table_build_device(rc_ctx *ctx, uint64_t *d_codes, const int32_t *d_counts, size_t n);
/* replaces main.cpp:294-308 including the parse: reads a `jellyfish dump` text file
 * (">COUNT\nKMER\n"), drops count <= 1, builds the table.  *stored = the "Stored %d kmers" value. */
int rc_table_load_jfdump(rc_ctx *ctx, const char *path, int64_t *stored);
/* replace stages 0-2 (run_rcorrector.pl:262-281: jellyfish bc / count -C / dump -L 2): exact
 * canonical k-mer counts over any number of arenas of reads (reads separated by NUL bytes, each
 * arena < 2^32 bytes; k-mers holding a letter outside ACGT are skipped), then the table from the
 * entries with count >= min_count.  count_add takes a host arena, count_add_device one already in
 * HBM.  *n_kmers = entries kept (the "Stored %d kmers" value).  The kept entries' codes (8 bytes each) stay in HBM behind
 * the table for rc_estimate_error_rate, which reads them instead of decoding the buckets and frees them; a caller that
 * never estimates gets the memory back at rc_set_run_params (or with the table). */
int rc_table_count_begin(rc_ctx *ctx);
int rc_table_count_add(rc_ctx *ctx, const char *seq, size_t nbytes);
int rc_table_count_add_device(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes);
int rc_table_count_finish(rc_ctx *ctx, int min_count, int64_t *n_kmers);
/* on != 0: rc_table_count_finish leaves the arenas it was given in HBM (in the order of the non-empty count_add calls)
 * instead of releasing them, for rc_submit_resident below: a data set whose k-mers were counted on this GPU is corrected
 * where it lies and crosses PCIe once.  rc_table_count_arenas reports how many there are (and the bytes of the first
 * `cap`); they are released by the next rc_table_count_begin, by rc_table_count_release, or with the context. */
int rc_table_count_keep(rc_ctx *ctx, int on);
int rc_table_count_arenas(const rc_ctx *ctx, size_t *n_arenas, uint64_t *bytes, size_t cap);
int rc_table_count_release(rc_ctx *ctx);
/* ends a session opened by rc_table_count_begin WITHOUT counting: the arenas added since stay in HBM as kept arenas (in the
 * order of the non-empty count_add calls), no table is built and the context's table, if any, stays.  For a GPU that will
 * correct reads whose k-mers another GPU counts (the table arrives by rc_table_replicate): one Store, T workers,
 * main.cpp:294-308,451 -- each worker's reads uploaded once, to the GPU that corrects them. */
int rc_table_count_park(rc_ctx *ctx);
/* rc_table_count_finish for reads that are spread over n contexts, one per GPU -- each with a session of its own
 * (rc_table_count_begin, count_add of the reads THAT GPU will correct): the key space is cut into the slices one GPU would
 * use, slice p belongs to ctxs[p % n]; every GPU emits a slice's keys from its own arenas and sends them to the owner
 * (peer to peer where the GPUs can, else through the host), which sorts and reduces them; the entries with count >=
 * min_count are put end to end in slice order on ctxs[0], where the table is built -- the same entries in the same order
 * as one GPU holding all the reads would produce (ERROR_RATE and rc_table_write_jfdump depend on the order); the other
 * contexts get the table by rc_table_replicate.  ctxs[0]'s rc_table_count_keep setting applies to every context (the
 * arenas stay where they are for rc_submit_resident).  One Store for T workers, main.cpp:294-308, counted by all of them. */
int rc_table_count_finish_sharded(rc_ctx **ctxs, int n, int min_count, int64_t *n_kmers);
/* begin + add_device + finish for one arena */
int rc_table_count_reads_device(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, int min_count,
                                int64_t *n_kmers);
/* the table as the text `jellyfish dump` writes (">COUNT\nKMER\n", canonical k-mers) -- the file
 * main.cpp:295-307 parses -- so a table counted here can be handed to the reference binary.
 * Entries are written in "dump order" (ascending splitmix64 of the code: pseudo-random like
 * Jellyfish's hash order, but reproducible). */
int rc_table_write_jfdump(rc_ctx *ctx, const char *path, int64_t *n_written);
/* dst uses src's table (same device; src must outlive dst and must not rebuild its table meanwhile).
 * The reference shares one Store between all worker threads (main.cpp:451); this lets several
 * contexts -- several batches in flight on one GPU -- do the same instead of replicating it. */
int rc_table_share(rc_ctx *dst, const rc_ctx *src);
/* dst gets its own copy of src's table: the bucket array goes device to device (over xGMI when the
 * contexts sit on different GPUs) -- the replication step of a multi-GPU run; the dump is parsed and the
 * table built once (main.cpp:294-308 loads one Store for all workers).  rc_estimate_error_rate() keeps
 * working on src only (dst has no dump order of its own until asked: it falls back to the table's). */
int rc_table_replicate(rc_ctx *dst, const rc_ctx *src);
/* the same with the copy left in flight on dst's stream (rc_sync(dst) waits for it): a host replicating to the other
 * GPUs of a node queues all its copies first -- they travel over different xGMI links at the same time.  GPUs without
 * peer access to the source get their copy staged through page-locked host memory (then complete on return). */
int rc_table_replicate_async(rc_ctx *dst, const rc_ctx *src);
/* Store::GetCount (Store.h:59-66) for n valid k-mer codes (host arrays) */
int rc_table_lookup(rc_ctx *ctx, const uint64_t *codes, size_t n, int32_t *counts_out);
/* every stored (canonical code, count) pair, unspecified order -- what `jellyfish dump` would
 * print (run_rcorrector.pl:280); *n_out = number stored (may exceed cap: call again) */
int rc_table_export(rc_ctx *ctx, uint64_t *codes, int32_t *counts, size_t cap, size_t *n_out);
/* 64-bit digest of the table's content (every stored canonical code with its count; independent of
 * the bucket layout): equal digests = replicas that answer every Store::GetCount alike.  The
 * multi-GPU callers compare it across devices after replicating the table (main.cpp:294-308 loads ONE
 * Store for all workers). */
int rc_table_digest(rc_ctx *ctx, uint64_t *digest);
/* slot layout the last build chose: 0 = WIDE (5 x 12-byte {code, count} slots per 64-byte bucket, any k
 * and count), 1 = PACKED (8 x 8-byte {remainder, count} slots: the code is implied by the bucket it
 * hashes to; the count field has 27 bits, less up to 8 where a large k over a small table needs more
 * remainder bits, larger counts live in a side array of the same allocation; taken when at most 4000
 * counts overflow and the placement allows: a third less HBM per k-mer).
 * Same answers either way (rc_table_digest is layout independent).  < 0: no table. */
int rc_table_layout(const rc_ctx *ctx);
/* bytes of HBM held by the table, number of buckets, number of stored entries */
int rc_table_stats(const rc_ctx *ctx, uint64_t *bytes, uint64_t *buckets, uint64_t *entries);

/* ---- k-mer count spectrum (what `jellyfish histo` prints of a Jellyfish database) ---------------------------------------------
 * A spectrum with bound max_bin >= 1 is uint64_t freq[max_bin + 1]: freq[0] = 0; freq[c], 1 <= c < max_bin, the number of
 * distinct canonical k-mers whose count is exactly c; freq[max_bin] the number whose count is >= max_bin.  The statistics
 * are exact whatever max_bin is (total = the sum of the counts).  No reference counterpart: the reference reads a
 * Jellyfish database, which `jellyfish histo` summarises; this library counts without one. */
typedef struct {
    uint64_t distinct, total, unique, max_count;
} rc_spectrum_stats;
/* arms the counted spectrum with bound max_bin (0 = off, the default; at most 2^28): the next rc_table_count_finish /
 * rc_table_count_finish_sharded (ctxs[0]'s setting, result on ctxs[0]) bins every canonical k-mer it sees -- those below
 * min_count included, with its full 32-bit count; k-mers holding a letter outside ACGT are left out, as by the counter.  The
 * setting stays until changed; the result stays in host memory until the next rc_table_count_begin. */
int rc_table_count_spectrum(rc_ctx *ctx, uint32_t max_bin);
/* source 0: the live entries of the current table (the counts rc_table_lookup returns; any table: counted, loaded, built,
 * shared or replicated) -- RC_STATUS_STATE without a table.  source 1: the counted spectrum of the last finish, folded
 * into max_bin if that is below its bound -- RC_STATUS_STATE if none was armed, RC_STATUS_ARG above the armed bound.
 * stats may be NULL. */
int rc_table_spectrum(rc_ctx *ctx, int source, uint64_t *freq, uint32_t max_bin, rc_spectrum_stats *stats);

/* ---- two tables side by side: the joint count matrix of their k-mers (what `kat comp` computes from two Jellyfish hashes) ------
 * cells is the caller's array of (max_bin + 1)^2 words, max_bin 1 .. 1023 (at most 8 MiB on the device: a limit of this
 * call): cells[i * (max_bin + 1) + j] = the number of distinct canonical k-mers whose count in a's table folds to i and
 * whose count in b's folds to j -- folded as rc_table_spectrum folds (exact below max_bin, the last bin "at least
 * max_bin"), bin 0 = the table does not hold the k-mer; cells[0] = 0.  An entry is what rc_table_spectrum(source 0)
 * counts: a live entry with the count rc_table_lookup returns (the full count of a PACKED table's prefix included).  The
 * statistics are exact whatever max_bin is; stats may be NULL.
 * Any two tables of the same k on the same device: built, loaded, counted, shared (rc_table_share) or replicated, of any
 * layout each; a == b is allowed (a diagonal matrix).  Both contexts are drained first (their queued batches complete);
 * the kernels run on a's stream and the call is complete on return.  Neither table is changed (rc_table_digest stays).
 * RC_STATUS_STATE: a context without a table.  RC_STATUS_ARG: different k, contexts on different devices (bring one
 * table over with rc_table_replicate), cells NULL, max_bin out of range.  The error text is a's (rc_last_error(a)).
 * No reference counterpart. */
typedef struct {
    uint64_t distinct_a, distinct_b, shared;   /* distinct canonical k-mers; shared = held by both */
    uint64_t mass_a, mass_b;                   /* sum of the counts (exact, not folded) */
    uint64_t shared_mass_a, shared_mass_b;     /* a's / b's counts summed over the shared k-mers */
    uint64_t max_count_a, max_count_b;
} rc_table_compare_stats;
int rc_table_compare(rc_ctx *a, rc_ctx *b, uint32_t max_bin, uint64_t *cells, rc_table_compare_stats *stats);

/* ---- recount session: the k-mer spectrum of reads AFTER correction, and a census of the k-mers the table does not hold ------
 * A second, read-only use of the k-mer counter.  Between rc_recount_begin and rc_recount_finish the session collects arenas of
 * reads (NUL-separated, each arena < 2^32 bytes) in HBM, one byte per base; finish counts them by the counter's rules -- canonical
 * k-mers at the context's k, windows holding a letter outside ACGT or crossing a NUL skipped, full 32-bit counts -- and probes
 * every distinct k-mer in the context's table.  freq is laid out as rc_table_spectrum documents (freq[0] = 0, last bin = "at
 * least"), with the max_bin given to begin (1 .. 2^28).  The session builds no table and never touches the one that is there
 * (rc_table_digest stays), releases and reorders no kept arena, leaves an armed or stored counted spectrum alone, and gives
 * the same answer in one pass as in several (RC_COUNT_MEM_MB).  RC_STATUS_STATE: begin / add / finish without a table, add /
 * finish without begin, begin while a session of either kind is open, rc_table_count_begin while this one is; RC_STATUS_ARG: a
 * bad max_bin.  finish, an error in add or finish, and rc_destroy end the session and leave nothing of it allocated.
 * No reference counterpart: there one runs Jellyfish over the corrected files. */
typedef struct {
    rc_spectrum_stats all;                  /* distinct, total, unique, max_count of the recounted k-mers */
    uint64_t absent_distinct, absent_total; /* of those, the k-mers the context's table does not hold (GetCount 0, Store.h:59-66):
                                               the number of distinct ones, and the sum of their counts */
} rc_recount_stats;
int rc_recount_begin(rc_ctx *ctx, uint32_t max_bin);
/* a host arena / an arena already in HBM (what rc_correct_device has corrected in place: the caller's memory); copied, the
 * caller's buffer is its own again on return.  No reference counterpart. */
int rc_recount_add(rc_ctx *ctx, const char *seq, size_t nbytes);
int rc_recount_add_device(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes);
/* on != 0 (default off): while a session is open on ctx, every batch that completes on it -- rc_correct_batch, rc_wait,
 * rc_wait_packed, rc_wait_resident, the batches of slots that run in lanes included -- appends its corrected byte arena to the
 * session, device to device on the batch's own stream, before the wait returns and the slot can be reused; each batch once.
 * Without a session, or with on == 0, those calls do exactly what they do without this one.  No reference counterpart. */
int rc_recount_follow(rc_ctx *ctx, int on);
/* freq[max_bin + 1] (begin's max_bin); stats may be NULL.  No reference counterpart. */
int rc_recount_finish(rc_ctx *ctx, uint64_t *freq, rc_recount_stats *stats);

/* ---- correction report: what was changed, where in the read, and in which reads ---------------------------------------------
 * While the report is armed on a context, every batch that completes on it -- rc_correct_batch, rc_correct_batch_traced,
 * rc_wait, rc_wait_packed, rc_wait_resident (the batches of slots that run in lanes included), rc_correct_device (in stream
 * order, at the end of the call) and rc_correct_read -- is compared on the GPU with a copy of its arena taken before the
 * first correction kernel, and every byte that differs (a correction only ever writes one of ACGT over a different byte,
 * ErrorCorrection.cpp:1468-1479) is counted below; each batch once: a packed or resident batch that came back with
 * RC_STATUS_NOSPACE is counted when its resubmission completes.  Not armed, those calls launch, copy and allocate nothing
 * for it; armed or not, the corrected reads, ret / l / m / h, rc_summary and rc_table_digest are the same.
 *   mate 0: every read of mode 0, the first half of a mode-1 arena, the even reads of mode 2; mate 1: the others.
 *   Positions are 0-based; a position (or length) of RC_REPORT_MAX_LEN - 1 or more is counted in the last entry (the
 *   reference's reads have at most 1023 bases, utils.h:7).
 *   subst[from][to]: from = 0..3 for the letters A C G T exactly as the kernels read them -- upper case only: a lower-case
 *   letter is to them a letter outside ACGT, and is counted like N and everything else in row 4 --, to = A C G T.
 *   by_qual: [0] the changed base was of low quality by the very test the correction applies (quality byte <=
 *   badQualityThreshold, or its quality bit clear), [1] of high quality, [2] the read came without qualities (its first
 *   quality byte is 0: FASTA, Reads.h:241).
 *   per_read[c]: reads with c changed bases, c = 0 included; the last entry: RC_REPORT_MAX_PER_READ or more.
 * begin: RC_STATUS_STATE if armed already (needs no table).  get: waits for the report kernels outstanding on the context and
 * its lanes, then copies the counts out; the report stays armed and goes on accumulating; RC_STATUS_STATE if not armed.
 * end: disarms and frees (rc_destroy does too); RC_STATUS_STATE if not armed; a packed / resident batch in flight across end is
 * in no report.  A byte batch (rc_submit) is counted once its kernels are queued, whether or not the caller waits for it.
 * Armed, the comparison reads the arena in aligned 16-byte pieces: rc_correct_device's d_seq is read (never written) up to
 * 15 bytes in front of its first and behind its last byte, within the 16-byte granules those bytes lie in.
 * No reference counterpart. */
#define RC_REPORT_MAX_LEN 1024
#define RC_REPORT_MAX_PER_READ 64
typedef struct {
    uint64_t reads[2];           /* reads seen */
    uint64_t reads_changed[2];   /* ... with at least one changed base */
    uint64_t reads_unfixable[2]; /* ... with ret == -1 */
    uint64_t changes[2];         /* changed bases */
    uint64_t len_hist[2][RC_REPORT_MAX_LEN]; /* reads by length (reads covering position p = the sum of the entries above p) */
    uint64_t by_pos5[2][RC_REPORT_MAX_LEN];  /* changes by distance from the read's first base */
    uint64_t by_pos3[2][RC_REPORT_MAX_LEN];  /* changes by distance from its last base (0 = the last base) */
    uint64_t subst[5][4];        /* changes by original letter (A C G T, other) and new letter (A C G T) */
    uint64_t by_qual[3];         /* changes on a low-quality base, on a high-quality base, in reads without qualities */
    uint64_t per_read[RC_REPORT_MAX_PER_READ + 1]; /* reads by number of changed bases */
} rc_change_report;
int rc_change_report_begin(rc_ctx *ctx);
int rc_change_report_get(rc_ctx *ctx, rc_change_report *out);
int rc_change_report_end(rc_ctx *ctx);

/* ---- per-read weak-k-mer profile: which reads are still bad, and at which end ----------------------------------------------
 * For one read of L bases, at the context's k, against the context's table, with a threshold min_count >= 1: window i
 * (0 <= i <= L - k; none if L < k) is VALID if its k bytes are all upper-case ACGT exactly as the kernels read letters (lower
 * case, N and anything else make it invalid), a valid window is SOLID if GetCount of its canonical k-mer (Store.h:59-66) is at
 * least min_count and WEAK otherwise; invalid windows are neither.
 *   weak        number of weak windows
 *   bad_prefix  start of the first solid window
 *   bad_suffix  L - (start of the last solid window + k)
 *   uncovered   L - the number of bases that lie in at least one solid window (gaps in the middle count)
 * A read without a solid window has bad_prefix = bad_suffix = uncovered = L; L = 0 gives four zeros.  So bad_prefix +
 * bad_suffix <= uncovered <= L where a solid window exists, and with min_count = 1 the sum of `weak` over an arena is
 * rc_recount_stats.absent_total of a recount of the same arena.  Nothing is trimmed, dropped or reordered: the numbers only
 * annotate.  No reference counterpart: the reference carries the fields (_Read::badPrefix / badSuffix, Reads.h:20) and the
 * output branch that prints them (Reads.h:396-412) but hard-wires both to 0 (Reads.h:371-372). */
typedef struct { int32_t weak, bad_prefix, bad_suffix, uncovered; } rc_read_weak;   /* 16 bytes per read */
/* The reads of an arena in HBM as they are (call it behind rc_correct_device for the corrected ones): d_out[r] for each of the
 * n_reads reads (read r the NUL-terminated string at d_off[r]; d_off has n_reads + 1 entries).  Asynchronous on the context's
 * stream, like rc_strong_threshold_device (rc_sync() to wait).  Needs a table; d_seq is never written, and may be read in
 * aligned 16-byte pieces up to 15 bytes in front of its first and behind its last byte, as the correction report does.
 * max_read_len is not used: the reduce takes one read per lane, which walks the plane words of a read of any length (reads
 * of very different lengths in one wavefront wait for its longest).  RC_STATUS_ARG: min_count < 1, a null pointer with
 * n_reads > 0; RC_STATUS_STATE: no table.  rc_profile_get's kernel 4 times it.
 * No reference counterpart: the dormant fields of Reads.h:20,371-372,396-412. */
int rc_weak_profile_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                           int32_t max_read_len, int32_t min_count, rc_read_weak *d_out);
/* One-shot: the NEXT batch submitted into `slot` (rc_submit / rc_submit_packed / rc_submit_resident, slots that run in lanes
 * included; rc_correct_batch is slot 0) also profiles its corrected reads, on the GPU behind its last correction kernel;
 * out[total] (indexed like ret / l / m / h) holds them when that batch's wait returns success.  The submit consumes the
 * registration whether it succeeds or not: a batch resubmitted after RC_STATUS_NOSPACE registers again.  out == NULL
 * withdraws (min_count is not looked at then).  A page-locked `out` (rc_host_alloc) is written by DMA, any other through the
 * slot's staging by the wait that succeeds: where the wait fails (RC_STATUS_NOSPACE), a page-locked `out` may already have
 * been written and its content means nothing, any other is untouched.  Without a
 * registration a submit launches, copies and allocates nothing for it, and with or without one the corrected reads, ret / l /
 * m / h, rc_summary and rc_table_digest are the same.  rc_correct_batch_traced takes no slot: it ignores a registration and
 * leaves it for the next submit.  RC_STATUS_ARG: min_count < 1, a bad slot; RC_STATUS_STATE: no table.
 * No reference counterpart: the dormant fields of Reads.h:20,371-372,396-412. */
int rc_weak_profile_into(rc_ctx *ctx, int slot, rc_read_weak *out, int32_t min_count);

/* ---- per-read k-mer depth: the quartiles of every read's k-mer counts ----------------------------------------------------------
 * What digital normalisation and depth-aware filters ask of every read (Trinity's in-silico normalisation, khmer's
 * normalize-by-median): the median abundance of its k-mers.  For one read of L bases, at the context's k, against the
 * context's table: window i (0 <= i <= L - k; none if L < k) is VALID exactly as for rc_read_weak above, and a valid window's
 * count is GetCount of its canonical k-mer (Store.h:59-66), 0 for a k-mer the table does not hold -- a table loaded from a dump
 * written with a lower count bound (jellyfish dump -L 2) holds no k-mer seen once.  With n the number of valid windows and
 * c[0] <= ... <= c[n-1] their counts in ascending order:
 *   valid   n
 *   q1      c[(n - 1) / 4]
 *   median  c[(n - 1) / 2]
 *   q3      c[3 * (n - 1) / 4]      (integer division: lower quantiles, values that occur in the read)
 * and four zeros for n == 0.  q1 <= median <= q3.  Exact integer arithmetic: no floats, no sampling, no histogram bins.
 * Nothing is trimmed, dropped or reordered: the numbers only annotate.  No reference counterpart. */
typedef struct { int32_t valid, q1, median, q3; } rc_read_depth;   /* 16 bytes per read */
/* The reads of an arena in HBM as they are (call it behind rc_correct_device for the corrected ones): d_out[r] for each of the
 * n_reads reads (read r the NUL-terminated string at d_off[r]; d_off has n_reads + 1 entries).  Asynchronous on the context's
 * stream, like rc_weak_profile_device (rc_sync() to wait).  Needs a table; d_seq is never written, may start at any byte, and
 * may be read in aligned 4-byte pieces up to 15 bytes in front of its first and behind its last byte.  An offset pair that
 * leaves the arena describes no read and gives four zeros.  max_read_len is only checked: the kernel packs reads into its
 * tiles by their own lengths, and a read of more than 1 023 bases -- which max_read_len promised not to exist -- gives four
 * zeros.  RC_STATUS_ARG: a null pointer with n_reads > 0, an arena of 4 GiB or more, max_read_len above the library's 1 023
 * bases; RC_STATUS_STATE: no table.  rc_profile_get's kernel 7 times it. */
int rc_read_depth_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                         int32_t max_read_len, rc_read_depth *d_out);
/* One-shot, as rc_weak_profile_into and under the same rules: the NEXT batch submitted into `slot` also takes the depth of its
 * corrected reads, on the GPU behind its last correction kernel; out[total] (indexed like ret / l / m / h) holds them when
 * that batch's wait returns success.  The submit consumes the registration whether it succeeds or not; out == NULL withdraws;
 * a page-locked `out` is written by DMA, any other by the wait that succeeds.  Both registrations may be armed on one submit.
 * Without one a submit launches, copies and allocates nothing for it.  RC_STATUS_ARG: a bad slot; RC_STATUS_STATE: no table. */
int rc_read_depth_into(rc_ctx *ctx, int slot, rc_read_depth *out);

/* ---- per-read screen: which reads hold the k-mers of a second set -------------------------------------------------------------
 * rc_table_compare says how much of a library's k-mer mass an rRNA, mitochondrial, adapter or host set holds; this says which
 * reads hold it -- the step taken right after correction (rRNA removal, host or PhiX decontamination), without a second aligner
 * run: the reads are in HBM already, and the work is one probe per base into a second table.  For one read of L bases, at the
 * context's k, against the table S of another context (the SCREEN context; it may be the same one) and a threshold min_count
 * >= 1: window i (0 <= i <= L - k; none if L < k) is VALID exactly as for rc_read_weak above, and a valid window is a HIT if
 * GetCount of its canonical k-mer in S (Store.h:59-66) is at least min_count.
 *   valid    number of valid windows
 *   hits     number of hit windows
 *   covered  number of bases of the read that lie inside at least one hit window, 0 .. L
 *   longest  the longest run of consecutive window positions that are all hits (an invalid window is no hit and ends a run);
 *            such a run spans longest + k - 1 bases
 * and four zeros for a read shorter than k.  hits <= valid, longest <= hits, and with hits > 0: longest + k - 1 <= covered <=
 * min(L, hits * k).  Nothing is trimmed, dropped or reordered: the numbers only annotate.  No reference counterpart. */
typedef struct { int32_t valid, hits, covered, longest; } rc_read_screen;   /* 16 bytes per read */
/* The reads of an arena in HBM as they are (call it behind rc_correct_device for the corrected ones): d_out[r] for each of the
 * n_reads reads, under rc_read_depth_device's rules for d_seq, d_off, offsets that leave the arena and max_read_len.
 * Asynchronous on ctx's stream (rc_sync(ctx) to wait).  ctx supplies k, device and stream and needs no table of its own;
 * `screen` must hold a table -- built, loaded, counted, shared or replicated, of either slot layout, whatever ctx's own is -- of
 * the same k on the same device, is not changed, and must keep that table until the kernel has run.  RC_STATUS_ARG: a null
 * pointer (screen; the others with n_reads > 0), an arena of 4 GiB or more, max_read_len above the library's 1 023 bases,
 * min_count < 1, a screen context of another k or on another device; RC_STATUS_STATE: no table in `screen`.  rc_profile_get's
 * kernel 8 (of ctx) times it. */
int rc_read_screen_device(rc_ctx *ctx, const rc_ctx *screen, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads,
                          uint64_t nbytes, int32_t max_read_len, int32_t min_count, rc_read_screen *d_out);
/* One-shot, as rc_weak_profile_into and under the same rules: the NEXT batch submitted into `slot` also has its corrected
 * reads screened against `screen`'s table, on the GPU behind its last correction kernel; out[total] (indexed like ret / l / m
 * / h) holds them when that batch's wait returns success.  The submit consumes the registration whether it succeeds or not;
 * out == NULL withdraws (screen and min_count are not looked at then); a page-locked `out` is written by DMA, any other by the
 * wait that succeeds.  It may be armed together with the weak profile and the depth on one submit; one screen set per
 * registration.  THE SCREEN CONTEXT AND ITS TABLE MUST STAY ALIVE AND UNCHANGED UNTIL THAT BATCH'S WAIT HAS RETURNED: the
 * kernel reads the table where it lies.  Without a registration a submit launches, copies and allocates nothing for it.
 * RC_STATUS_ARG: a bad slot, and with out != NULL a null screen, min_count < 1, another k or another device;
 * RC_STATUS_STATE: no table in `screen`. */
int rc_read_screen_into(rc_ctx *ctx, int slot, const rc_ctx *screen, int32_t min_count, rc_read_screen *out);

/* ---- normalisation by k-mer depth: which reads or pairs to keep so that no transcript is covered much beyond a target ---------
 * What an assembler does first with corrected reads (in-silico normalisation): count the k-mers, take every read's median k-mer
 * coverage, keep a unit with probability target / median.  The counter and rc_read_depth are the two expensive stages; this is
 * the selection.  The scheme is after Trinity's normalisation with --pairs_together -- the mates' medians averaged, a unit kept
 * with max_cov / median -- but neither its random stream nor byte parity with it is claimed, and its coefficient-of-variation
 * filter has no counterpart.  A UNIT is a read (mode 0), read u with read n_units + u (mode 1) or reads 2u and 2u + 1 (mode 2):
 * the duplicate census's modes.
 *   depth D   of the rc_read_depth of the unit's mates, those with valid > 0 only: one such mate -- its median; two --
 *             (m1 + m2 + 1) >> 1, unsigned; none -- the unit is NOVALID
 *   draw r    z = seed + (index + 1) * 0x9E3779B97F4A7C15 through the splitmix64 finaliser (z ^= z >> 30, z *= 0xBF58476D1CE4E5B9,
 *             z ^= z >> 27, z *= 0x94D049BB133111EB, z ^= z >> 31), r its upper 32 bits; index = unit_base + u, 64 bits: the
 *             unit's number in the WHOLE input, not in the batch
 *   outcome   RC_NORM_NOVALID: no mate with valid > 0; else RC_NORM_LOW: D < min_cov; else RC_NORM_KEPT: D <= target or
 *             (uint64_t)r * D < (uint64_t)target << 32; else RC_NORM_OVER
 * A unit is kept with probability min(1, target / D) to within 2^-32, and the decision depends on (seed, index, D) alone: a run
 * is reproducible and the same however the input is cut into batches.  Integer arithmetic throughout (rc_norm.h).  No reference
 * counterpart. */
#define RC_NORM_OVER 0
#define RC_NORM_KEPT 1
#define RC_NORM_LOW 2
#define RC_NORM_NOVALID 3
/* d_depth: what rc_read_depth_device left in HBM, n_units entries in mode 0 and 2 * n_units in modes 1 and 2, on a 16-byte
 * boundary.  d_keep[u] = the outcome of unit u for u < n_units; no other byte is written.  d_tally: 4 + 2 * (max_bin + 1) words
 * in HBM that the call ADDS to -- it accumulates over batches, the caller zeroes it: the four outcome counts indexed by outcome
 * value, then before[min(D, max_bin)] over the units that are not NOVALID, then after[min(D, max_bin)] over the KEPT ones.
 * Asynchronous on the context's stream (rc_sync() to wait); ctx needs no table.  n_units == 0: RC_STATUS_OK, no launch.
 * RC_STATUS_ARG (checked whatever n_units is): a mode outside 0..2, target == 0 or >= 2^31, max_bin outside 1 .. 65535; with
 * n_units > 0: a null pointer, a misaligned d_depth or d_tally.  rc_profile_get's kernel 9 times it. */
int rc_norm_select_device(rc_ctx *ctx, const rc_read_depth *d_depth, uint32_t n_units, int mode, uint64_t unit_base, uint32_t target,
                          uint32_t min_cov, uint64_t seed, uint32_t max_bin, uint8_t *d_keep, uint64_t *d_tally);

/* ---- duplicate census: how many reads / pairs are exact copies of one another, before and after correction ------------------
 * A UNIT is a read (mode 0) or a pair (mode 1: read r of the first half and read r of the second; mode 2: reads 2u and 2u + 1 --
 * the mates of the correction report).  Two units are duplicates when their base strings are byte for byte equal: equal
 * length, N / lower case / any other byte compared as it is, mate 1 with mate 1 and mate 2 with mate 2 -- no reverse
 * complement, (a, b) is not (b, a), ("AC", "GT") is not ("ACG", "T"); qualities and names play no part.
 * While a census is open on a context, every batch that completes on it -- rc_correct_batch, rc_correct_batch_traced, rc_wait,
 * rc_wait_packed, rc_wait_resident (the batches of slots that run in lanes included) and rc_correct_device (in stream order,
 * at the end of the call) -- leaves one 128-bit key per unit and version: BEFORE, of the bases as they were in HBM in front of
 * the first correction kernel, and AFTER, of the bases as corrected (an unfixable read keeps its bases and counts like any
 * other).  Each batch once: a packed or resident batch that came back with RC_STATUS_NOSPACE counts when its resubmission
 * completes.  The keys of all batches stay in HBM, 16 bytes per unit and version, until end.  Equality is decided on the key
 * alone (two independent 64-bit hashes of the bytes, the chunk order, the length, the mate and the split between the mates:
 * rc_dups.h); two different units with one key would be counted as copies, which for n units happens with probability about
 * n^2 / 2^129.  No census open, those calls launch, copy and allocate nothing for it; open or not, the corrected reads,
 * ret / l / m / h, rc_summary and rc_table_digest are the same.
 *   units             units seen
 *   distinct_x        distinct units of version x
 *   copies_x[c]       c = 1 .. max_bin: distinct units that occur exactly c times; the last entry: max_bin times or more (as
 *                     rc_table_spectrum folds); copies_x[0] = 0.  The caller's arrays, max_bin + 1 entries each.
 * So sum(copies_x) == distinct_x, and sum(c * copies_x[c]) == units while nothing reached the last entry.
 * begin: RC_STATUS_STATE if open already (needs no table).  get: waits for what is outstanding on the context and its lanes,
 * sorts a copy of the keys and counts the runs; the keys stay, the census stays open and goes on accumulating, any number of
 * gets; RC_STATUS_STATE if not open, RC_STATUS_ARG: max_bin < 1 or a null pointer.  end: closes and frees (rc_destroy does
 * too); RC_STATUS_STATE if not open; a batch in flight across end is in no census.  Where the key buffers cannot grow, the
 * call that completes the batch returns RC_STATUS_NOSPACE with a message -- a census is never silently short.  A census holds
 * at most 2^32 - 1 units (its sort indexes them with 32 bits; 64 GiB of keys per version): the batch that would pass that
 * returns RC_STATUS_NOSPACE too.  While a census is open rc_correct_device BLOCKS: it returns when the batch's kernels have run
 * and its keys are in the census (without one it stays asynchronous); the waits block as they always do.  Threads: begin, get,
 * end and merge are the caller's to serialise against each other and against submits and waits on the same context; submits
 * and waits of different slots may run on different threads as before (the lanes append under a mutex).  Open, the key
 * kernel reads the arena in aligned 16-byte pieces: rc_correct_device's d_seq is read (never written) up to 15 bytes in front
 * of its first and behind its last byte, within the 16-byte granules those bytes lie in.  No reference counterpart. */
typedef struct {
    uint64_t units, distinct_before, distinct_after;
    uint64_t *copies_before, *copies_after; /* the caller's, max_bin + 1 entries each */
} rc_dup_census;
int rc_dup_census_begin(rc_ctx *ctx);
int rc_dup_census_get(rc_ctx *ctx, uint32_t max_bin, rc_dup_census *out);
int rc_dup_census_end(rc_ctx *ctx);
/* The keys of an arena in HBM as it is: d_keys[2 u], d_keys[2 u + 1] for unit u (n_reads reads, read r the NUL-terminated
 * string at d_off[r], d_off has n_reads + 1 entries; mode 0: n_reads units, modes 1 and 2: n_reads / 2).  Asynchronous on the
 * context's stream (rc_sync() to wait); needs neither a table nor an open census.  RC_STATUS_ARG: a mode outside 0..2, an odd
 * n_reads in modes 1 and 2, a null pointer with n_reads > 0, an arena of 4 GiB or more.  No reference counterpart. */
int rc_read_keys_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes, int mode, uint64_t *d_keys);
/* Appends the keys src has accumulated to dst's (both open; src keeps its own): device to device where the two are on one
 * device or peers, else through the host.  What several GPUs' contexts do at the end of a run.  RC_STATUS_STATE: either one
 * not open; RC_STATUS_ARG: dst == src.  No reference counterpart. */
int rc_dup_census_merge(rc_ctx *dst, rc_ctx *src);

/* ---- recurrent-correction census: one fix made in many reads --------------------------------------------------------------
 * A sequencing error lands at a random place; a real variant (a minor allele, an editing site, a paralogue's difference) is
 * rewritten into the dominant spelling in EVERY read that carries it.  The census names the sites where that happened.
 * A CHANGE is a position p of a read at which the byte of the arena as it arrived differs from the byte as corrected (the
 * corrected byte is one of upper-case ACGT, as the correction report relies on).  Its WINDOW is the RC_RECUR_FLANK = 14 bytes
 * on either side of it and the byte itself, the 29 bytes after[p - 14 .. p + 14] of the CORRECTED read -- the stable spelling:
 * neighbouring fixes have been applied to it too.  A change is CONTEXTED when p >= 14, p + 14 < L (L the read's length) and all
 * 29 window bytes are upper-case ACGT, exactly as the kernels read letters; every other change is CLIPPED: counted in the
 * totals, without a key.  The FROM code f is 0..3 when the original byte is upper-case A C G T, else 4 (N, lower case, ...: row
 * 4 of rc_change_report.subst).  The SITE KEY: W = the window, 2 bits a base (A C G T = 0 1 2 3), first base most significant,
 * 58 bits; the reverse strand sees the same event as W' = revcomp(W) with f' = 3 - f (4 stays 4); the window's length is odd, so
 * its centre stays the centre and W != W' always (no base is its own complement): the orientation with the smaller W is
 * canonical, and key = (W_canon << 3) | f_canon -- 61 bits, one uint64_t, 8 bytes per contexted change.  The new base is the
 * centre of W_canon (bits 32..31 of the key); rc_recur.h holds this arithmetic for device and host.
 * The census is the multiset of the keys of all contexted changes of the batches that completed while it was open -- the same
 * entry points as the duplicate census, each batch once (a packed or resident batch that came back with RC_STATUS_NOSPACE
 * counts when its resubmission completes); rc_correct_read is no batch of the run and is in none.  A SITE is a distinct key,
 * its count the changes with that key; changes in the two mates of a pair, or in two copies of a duplicate, count once each.
 * No census open, those calls launch, copy and allocate nothing for it; open or not, the corrected reads, ret / l / m / h,
 * rc_summary and rc_table_digest are the same.  The arena as it arrived is the copy the correction report takes (one copy for
 * the report, the mate-overlap session and this census, whichever are open).
 *   changes, contexted, clipped   contexted + clipped == changes; changes == changes[0] + changes[1] of an rc_change_report
 *                                 armed over the same batches
 *   sites                         distinct keys
 *   sites_recurrent               sites with two changes or more; changes_at_recurrent: their changes
 *   recur[c]                      c = 1 .. max_bin: sites with exactly c changes; the last entry: max_bin or more; recur[0] = 0.
 *                                 The caller's array, max_bin + 1 entries.  sum(recur) == sites
 *   n_top, top_key, top_count     the sites with min_count changes or more, by count descending, then key ascending -- all of
 *                                 them, or the first max_sites (exact, not sampled).  The caller's arrays, max_sites entries
 * begin: RC_STATUS_STATE if open already (needs no table).  get: waits for what is outstanding on the context and its lanes,
 * sorts a copy of the keys and counts the runs; the keys stay, the census stays open and goes on accumulating, any number of
 * gets; RC_STATUS_STATE if not open, RC_STATUS_ARG: max_bin < 1 (or above 2^28), min_count < 1, a null pointer (top_key /
 * top_count may be NULL with max_sites == 0).  end: closes and frees (rc_destroy does too); RC_STATUS_STATE if not open; a batch
 * in flight across end is in no census, and nothing staged for an ended census reaches the next one.  Where the key buffer
 * cannot grow, the call that completes the batch returns RC_STATUS_NOSPACE with a message -- a census is never silently short.
 * A census holds at most 2^32 - 1 keys (its sort indexes them with 32 bits; 32 GiB of keys): the batch that would pass that
 * returns RC_STATUS_NOSPACE too.  While a census is open every submit and rc_correct_device BLOCK until the batch's kernels have
 * run: how many keys a batch has is known only then, and the keys that did not fit the first launch's buffer are taken by a
 * second one while the snapshot is still there (without a census they stay asynchronous); the waits block as they always do.
 * Threads: as for the duplicate census.  Open, the key kernel reads both arenas in aligned 16-byte pieces: rc_correct_device's
 * d_seq is read (never written) up to 15 bytes in front of its first and behind its last byte, within the 16-byte granules
 * those bytes lie in.  No reference counterpart. */
#define RC_RECUR_FLANK 14
typedef struct {
    uint64_t changes, contexted, clipped;
    uint64_t sites, sites_recurrent, changes_at_recurrent;
    uint64_t *recur;                /* the caller's, max_bin + 1 entries */
    uint64_t *top_key, *top_count;  /* the caller's, max_sites entries each */
    uint32_t n_top;
} rc_recur_census;
int rc_recur_census_begin(rc_ctx *ctx);
int rc_recur_census_get(rc_ctx *ctx, uint32_t max_bin, uint32_t min_count, uint32_t max_sites, rc_recur_census *out);
int rc_recur_census_end(rc_ctx *ctx);
/* Appends the keys and totals src has accumulated to dst's (both open; src keeps its own): device to device where the two are
 * on one device or peers, else through the host.  RC_STATUS_STATE: either one not open; RC_STATUS_ARG: dst == src. */
int rc_recur_census_merge(rc_ctx *dst, rc_ctx *src);
/* The site keys of two arenas in HBM as they are: d_before and d_after hold the same n_reads reads (read r the NUL-terminated
 * string at d_off[r], d_off has n_reads + 1 entries) at the same alignment modulo 16.  The keys of the contexted changes are
 * appended to d_keys in no particular order, never past d_keys[cap - 1]; d_counts[0 .. 2] (in HBM, zeroed first) = changes,
 * contexted changes, keys found -- always exact: d_counts[2] > cap says how much room a second call needs.  Asynchronous on the
 * context's stream (rc_sync() to wait); needs neither a table nor an open census.  Both arenas are read (never written) in
 * aligned 16-byte pieces: up to 15 bytes in front of their first and behind their last byte, within the 16-byte granules
 * those bytes lie in; nothing read there reaches a key or a count.  RC_STATUS_ARG: a null pointer (d_keys may be NULL with
 * cap == 0, the arenas and d_off with n_reads == 0), d_keys or d_counts not 8-byte aligned, arenas of different alignment
 * modulo 16, an arena of 4 GiB or more.  No reference counterpart. */
int rc_change_keys_device(rc_ctx *ctx, const uint8_t *d_before, const uint8_t *d_after, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                          uint64_t *d_keys, uint64_t cap, uint64_t *d_counts);

/* ---- k-mer trust profile by read position: where along the reads the untrusted k-mers lie, before and after correction ------
 * Window validity, SOLID and WEAK are exactly those of the per-read weak-k-mer profile above (rc_read_weak): at the context's
 * k, against the context's table, at a threshold min_count >= 1.  A read of L bases has nwin = max(0, L - k + 1) windows;
 * window i has position p5 = i from the 5' end and p3 = nwin - 1 - i from the 3' end (p3 = 0 is the last window).  A MATE is
 * the correction report's: mode 0: every read is mate 0; mode 1: the first half of the reads is mate 0, the second half mate
 * 1; mode 2: even reads are mate 0, odd reads mate 1.  One rc_trust_counts describes one version of the reads; per mate m:
 *   windows[m][p]              reads that have a window p (nwin > p) -- the same number from either end
 *   solid5[m][p], weak5[m][p]  reads whose window at p5 = p is solid / weak
 *   solid3[m][p], weak3[m][p]  reads whose window at p3 = p is solid / weak
 * so the invalid windows at p are windows - solid - weak, sum(solid5[m]) == sum(solid3[m]) and sum(weak5[m]) == sum(weak3[m]),
 * and with min_count = 1 the sum of weak5 over an arena is the sum of rc_read_weak.weak over it (rc_recount_stats.absent_total
 * of a recount of it).  A read has at most RC_TRUST_MAX_LEN windows counted (the reference's reads have at most 1023 bases,
 * utils.h:7).  The profile only counts: nothing is trimmed, dropped or reordered.
 * While a profile is open on a context, every batch that completes on it -- rc_correct_batch, rc_correct_batch_traced,
 * rc_wait, rc_wait_packed, rc_wait_resident (the batches of slots that run in lanes included) and rc_correct_device (in
 * stream order, at the end of the call) -- counts once: BEFORE from the bases as they were in HBM in front of the first
 * correction kernel, AFTER from the bases as corrected (an unfixable read keeps its bases and counts like any other).  A
 * packed or resident batch that came back with RC_STATUS_NOSPACE counts when its resubmission completes.  No profile open,
 * those calls launch, copy and allocate nothing for it; open or not, the corrected reads, ret / l / m / h, rc_summary and
 * rc_table_digest are the same.
 * begin: RC_STATUS_STATE if open already or without a table (min_count means nothing without one), RC_STATUS_ARG: min_count <
 * 1.  get: waits for what is outstanding on the context and its lanes, then copies the counts out; the profile stays open
 * and goes on accumulating, any number of gets; RC_STATUS_STATE if not open, RC_STATUS_ARG: out == NULL.  end: closes and
 * frees (rc_destroy does too); RC_STATUS_STATE if not open; a batch in flight across end is in no profile.  While a profile
 * is open rc_correct_device BLOCKS: it returns when the batch's kernels have run and its counts are in the profile (without
 * one it stays asynchronous); the waits block as they always do.  Threads: begin, get and end are the caller's to serialise
 * against each other and against submits and waits on the same context; submits and waits of different slots may run on
 * different threads as before (the lanes add under a mutex).  Open, the planes kernel reads the arena in aligned 16-byte
 * pieces: rc_correct_device's d_seq is read (never written) up to 15 bytes in front of its first and behind its last byte,
 * within the 16-byte granules those bytes lie in.  -weak-ends and a profile each pay their own pass over the arena.
 * No reference counterpart. */
#define RC_TRUST_MAX_LEN 1024
typedef struct {                       /* one version of the reads */
    uint64_t windows[2][RC_TRUST_MAX_LEN]; /* [mate][p]: reads that have a window p (nwin > p); the same from either end */
    uint64_t solid5[2][RC_TRUST_MAX_LEN], weak5[2][RC_TRUST_MAX_LEN];   /* by p5 */
    uint64_t solid3[2][RC_TRUST_MAX_LEN], weak3[2][RC_TRUST_MAX_LEN];   /* by p3 */
} rc_trust_counts;                     /* invalid windows at p = windows - solid - weak */
typedef struct { int32_t k, min_count; uint64_t reads[2]; rc_trust_counts before, after; } rc_trust_profile;
/* The reads of an arena in HBM as they are: n_reads reads, read r the NUL-terminated string at d_off[r], d_off has n_reads + 1
 * entries, mates by `mode` as above; their counts are ADDED to *d_counts, an rc_trust_counts in HBM that the caller zeroed
 * (or that holds earlier arenas' counts).  Asynchronous on the context's stream, like rc_weak_profile_device (rc_sync() to
 * wait); needs a table, no open profile.  d_seq is never written, and may be read in aligned 16-byte pieces up to 15 bytes
 * in front of its first and behind its last byte, as the correction report and the weak profile do.  max_read_len, the
 * longest read in bases, picks the kernel instance (reads of up to 256 windows keep their counters in a quarter of the
 * registers); the kernel clamps every read's nwin to what the instance holds, at most RC_TRUST_MAX_LEN, so a wrong
 * max_read_len can never index outside the arrays -- a read longer than it said merely has only its first windows counted.
 * RC_STATUS_ARG: min_count < 1, a null pointer with n_reads > 0, a mode outside 0..2, mode 1 with an odd n_reads,
 * max_read_len > RC_TRUST_MAX_LEN - 1, nbytes >= 2^32; RC_STATUS_STATE: no table.  rc_profile_get's kernels 5 (the planes) and
 * 6 (accumulate and column sums) time it.  No reference counterpart. */
int rc_trust_profile_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                            int32_t max_read_len, int32_t mode, int32_t min_count, rc_trust_counts *d_counts);
int rc_trust_profile_begin(rc_ctx *ctx, int32_t min_count);
int rc_trust_profile_get(rc_ctx *ctx, rc_trust_profile *out);
int rc_trust_profile_end(rc_ctx *ctx);

/* ---- mate-overlap report: where the two mates of a pair disagree, before and after correction ------------------------------
 * Evidence that does not come from the k-mer table: where a fragment is shorter than its two reads together, mate 1 and the
 * reverse complement of mate 2 cover some bases twice, and a base they disagree on is a sequencing error in one of them.
 * A PAIR is (a, b), mate 1 of La bytes and mate 2 of Lb bytes; mode 1: read r of the first half of the reads with read r of the
 * second half, mode 2: reads 2u and 2u + 1 (the mates of the duplicate census); mode 0 has no pairs.  A base is VALID if it is
 * upper-case A, C, G or T.  r is the reverse complement of b: r[j] = comp(b[Lb - 1 - j]), A <-> T, C <-> G, any other byte
 * invalid.  For an OFFSET d in [-(Lb - 1), La - 1], a[i] faces r[i - d] for i in [max(0, d), min(La, d + Lb)); v(d) is the number
 * of faced positions where both bases are valid, m(d) the number of those where they differ.  d is ACCEPTED if
 * v(d) >= min_overlap and 100 m(d) <= max_mismatch_pct v(d) (integers).  The CHOSEN offset d* is the accepted one with the
 * largest v, then the smallest m, then the smallest d.  d* is decided on the bases as they arrived and applied unchanged to the
 * corrected bases (corrections are substitutions: the lengths are equal).  A pair without an accepted offset is not
 * overlapping and adds to `pairs` alone.  The fragment length is F = d* + Lb; d* < 0 is read-through.  Of a mate longer than
 * 1023 bases (the reference's reads hold no more, utils.h:7) the first 1023 are looked at.
 *   pairs, overlapping
 *   compared_x, disagree_x     the sums of v and m at d*, in version x
 *   resolved                   positions valid-and-different before, valid-and-equal after
 *   introduced                 positions valid-and-equal before, valid-and-different after: probable miscorrections
 *   kept                       positions that differ in both versions (one whose validity changes is in none of the three)
 *   pairs_improved / _worsened / _same   overlapping pairs with m after below / above / equal to m before
 *   frag[F]                    overlapping pairs by fragment length, F in 1 .. 2046
 *   compared5[mate][p], disagree5_before[mate][p], disagree5_after[mate][p]   by position from the 5' end of that mate: mate 1
 *                              p = i, mate 2 p = Lb - 1 - (i - d*), its index in b; compared5 counts the positions valid before
 * so sum(frag) == overlapping == pairs_improved + pairs_worsened + pairs_same, sum(compared5[0]) == sum(compared5[1]) ==
 * compared_before, sum(disagree5_x[0]) == sum(disagree5_x[1]) == disagree_x, and disagree_before == resolved + kept + (the
 * positions that differ before and are invalid after).  A low-complexity pair (a homopolymer, a short repeat) may be given an
 * offset that is not its fragment's; min_overlap 30 and max_mismatch_pct 10 keep that rare.
 * While a session is open on a context, every batch of pairs that completes on it -- rc_correct_batch, rc_correct_batch_traced,
 * rc_wait, rc_wait_packed, rc_wait_resident (the batches of slots that run in lanes included) and rc_correct_device (in
 * stream order, at the end of the call) -- counts once, its bases as they were in HBM in front of the first correction kernel
 * (one copy of the arena, shared with the correction report where both are open) against its bases as corrected.  A packed or
 * resident batch that came back with RC_STATUS_NOSPACE counts when its resubmission completes; a single-end batch (mode 0) adds
 * nothing.  No session open, those calls launch, copy and allocate nothing for it; open or not, the corrected reads, ret / l /
 * m / h, rc_summary and rc_table_digest are the same.  Needs no table.
 * begin: RC_STATUS_STATE if open already, RC_STATUS_ARG: min_overlap outside 1 .. 1023, max_mismatch_pct outside 0 .. 50.  get:
 * waits for what is outstanding on the context and its lanes, then copies the counts out; the session stays open and goes on
 * accumulating; RC_STATUS_STATE if not open, RC_STATUS_ARG: out == NULL.  end: closes and frees (rc_destroy does too);
 * RC_STATUS_STATE if not open; a batch in flight across end is in no session.  While a session is open rc_correct_device BLOCKS
 * until the batch's counts are in the session.  Threads: as for the trust profile (the lanes add under a mutex).  Open, the
 * kernel reads the arena in aligned 16-byte pieces: rc_correct_device's d_seq is read (never written) up to 15 bytes in front
 * of its first and behind its last byte, within the 16-byte granules those bytes lie in.  No reference counterpart. */
#define RC_OVERLAP_MAX_LEN 1024
#define RC_OVERLAP_FRAG_LEN 2048
typedef struct {
    uint64_t min_overlap, max_mismatch_pct; /* the session's (rc_mate_overlap_get); rc_mate_overlap_device leaves them alone */
    uint64_t pairs, overlapping;
    uint64_t compared_before, disagree_before, compared_after, disagree_after;
    uint64_t resolved, introduced, kept;
    uint64_t pairs_improved, pairs_worsened, pairs_same;
    uint64_t frag[RC_OVERLAP_FRAG_LEN];
    uint64_t compared5[2][RC_OVERLAP_MAX_LEN], disagree5_before[2][RC_OVERLAP_MAX_LEN], disagree5_after[2][RC_OVERLAP_MAX_LEN];
} rc_mate_overlap;
/* The pairs of two arenas in HBM that share one offset array: n_reads reads, read r the NUL-terminated string at d_off[r] of
 * d_before (the bases as read) and of d_after (as corrected), d_off has n_reads + 1 entries; their counts are ADDED to
 * *d_counts, an rc_mate_overlap in HBM that the caller zeroed (or that holds earlier arenas' counts).  d_before == d_after is
 * allowed: nothing was corrected, every after figure equals its before figure.  Asynchronous on the context's stream
 * (rc_sync() to wait); needs neither a table nor an open session.  Neither arena is written; both may be read in aligned 16-byte
 * pieces up to 15 bytes in front of their first and behind their last byte.  max_read_len, the longest read in bases, picks
 * the kernel instance (up to 256 bases, or up to 1023); the kernel cuts every mate to what its instance holds, so a wrong
 * max_read_len can never index outside the arrays -- a mate longer than it said merely has only its first bases looked at.
 * RC_STATUS_ARG: a mode outside 1 .. 2, an odd n_reads, min_overlap outside 1 .. 1023, max_mismatch_pct outside 0 .. 50,
 * nbytes >= 2^32, a null pointer with n_reads > 0.  No reference counterpart. */
int rc_mate_overlap_device(rc_ctx *ctx, const uint8_t *d_before, const uint8_t *d_after, const uint32_t *d_off, uint32_t n_reads,
                           uint64_t nbytes, int32_t max_read_len, int32_t mode, int32_t min_overlap, int32_t max_mismatch_pct,
                           rc_mate_overlap *d_counts);
int rc_mate_overlap_begin(rc_ctx *ctx, int32_t min_overlap, int32_t max_mismatch_pct);
int rc_mate_overlap_get(rc_ctx *ctx, rc_mate_overlap *out);
int rc_mate_overlap_end(rc_ctx *ctx);

/* ---- read trimming: how many bases of every read to keep -------------------------------------------------------------------
 * The step between a corrector and an assembler that recipes hand to a separate CPU program: a 3' quality cut, a 3' adapter
 * cut, and for pairs the cut of a mate that ran through a short fragment into the adapter.  For a read of L bases (at most 1023)
 * three independent cuts are taken on the read AS GIVEN, each a position in 0 .. L, L meaning "no cut" (rc_trim.h, integer
 * arithmetic throughout):
 *   cut_qual     BWA's and cutadapt's 3' rule at q = qual_min: S(i) = the sum over j >= i of q - (Q[j] - qual_base), S(L) = 0; i0 =
 *                the largest i with S(i) < 0 (-1: none); the cut is the largest i in (i0, L] at which S is maximal.  The stop at i0
 *                is part of the rule: a bad head behind a good middle is not trimmed.  qual_min = 0 or d_qual = NULL: L
 *   cut_adapter  adapter1 for mate 1, adapter2 for mate 2 (single reads are mate 1), 0 .. 64 bases of upper-case ACGT, length 0
 *                switches the cut off.  At offset d in 0 .. L - 1 read position i faces adapter base i - d; v(d) = the faced
 *                positions whose read base is upper-case ACGT, m(d) = those of them that differ; d is accepted if
 *                v >= adapter_min and 100 m <= adapter_mm_pct v; the cut is the smallest accepted d, else L.  Hamming only
 *   cut_pair     modes 1 and 2 with pair_overlap != 0: d* chosen exactly as the mate-overlap report chooses it (above) with
 *                pair_min_overlap and pair_mm_pct, over the bases as given; F = d* + Lb is the fragment's length, mate 1 keeps
 *                min(La, F) bases and mate 2 min(Lb, Lb + d*).  No accepted offset: L
 *   keep_len     min(cut_qual, cut_adapter, cut_pair)
 * A UNIT (a read in mode 0; read u with read n_reads / 2 + u in mode 1; reads 2u and 2u + 1 in mode 2: the duplicate census's
 * modes) is KEPT if every mate has keep_len >= min_len, else it is SHORT: a short mate drops its partner too.  Nothing is cut
 * or dropped here: the call says where to cut.  Not in scope: a compacted, trimmed arena written on the device, 5' trimming,
 * indels in the adapter alignment, a slot-transport registration.  No byte parity with cutadapt, TrimGalore or fastp is claimed.
 * No reference counterpart. */
typedef struct { int32_t keep_len, cut_qual, cut_adapter, cut_pair; } rc_read_trim;        /* 16 bytes per read */
typedef struct {
    int32_t qual_min, qual_base, adapter_min, adapter_mm_pct, pair_overlap, pair_min_overlap, pair_mm_pct, min_len;
    uint8_t adapter1[64], adapter2[64];
    int32_t adapter1_len, adapter2_len;
} rc_trim_params;
typedef struct {
    uint64_t reads[2];           /* by mate */
    uint64_t cut_reads[2][3];    /* [mate][quality, adapter, pair]: the reads whose cut is below L */
    uint64_t bases_removed[2];   /* the sum of L - keep_len */
    uint64_t short_reads[2];     /* the reads with keep_len < min_len */
    uint64_t units, units_kept;
    uint64_t pairs_overlapping;  /* the pairs with an accepted offset */
    uint64_t keep_hist[2][1024]; /* [mate][keep_len], every read, of kept and of short units alike */
} rc_trim_tally;
/* The reads of an arena in HBM: read r the NUL-terminated string at d_off[r] of d_seq, and of d_qual (may be NULL) its quality
 * bytes; d_off has n_reads + 1 entries.  d_out[r] = the rc_read_trim of read r; d_keep (may be NULL): one byte per unit, 1 kept,
 * 0 short; d_tally (may be NULL): an rc_trim_tally in HBM that the call ADDS to -- the caller zeroes it.  Asynchronous on the
 * context's stream (rc_sync() to wait); needs no table.  Neither arena is written; both may be read in aligned 16-byte pieces up
 * to 15 bytes in front of their first and behind their last byte.  max_read_len, the longest read in bases, picks the kernel
 * instance (up to 256 bases, or up to 1023); a mate longer than its instance holds is cut to that first, so a wrong max_read_len
 * can never index outside the arrays.  n_reads == 0: RC_STATUS_OK, no launch.  RC_STATUS_ARG (checked whatever n_reads is): a
 * mode outside 0 .. 2, an odd n_reads in modes 1 and 2, params == NULL, nbytes >= 2^32, max_read_len outside 0 .. 1023, qual_min
 * outside 0 .. 93, qual_base outside 0 .. 255, adapter_min outside 1 .. 64, adapter_mm_pct or pair_mm_pct outside 0 .. 50,
 * pair_min_overlap outside 1 .. 1023, min_len outside 0 .. 1023, an adapter length outside 0 .. 64 or an adapter base outside
 * ACGT; with n_reads > 0: d_seq, d_off or d_out NULL, d_out off a 4-byte or d_tally off an 8-byte boundary. */
int rc_read_trim_device(rc_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                        int32_t max_read_len, int32_t mode, const rc_trim_params *params, rc_read_trim *d_out, uint8_t *d_keep,
                        rc_trim_tally *d_tally);

/* ---- read merging: one fragment-long read from two overlapping mates, written on the device ---------------------------------
 * What an overlap is most often used for, and what recipes hand to FLASH, PEAR, BBMerge or fastp --merge.  A pair is a (mate 1,
 * La bases) and b (mate 2, Lb bases); r is the reverse complement of b and at offset d, a[i] faces r[i - d] (the mate-overlap
 * report, above).  d* is chosen exactly as that report and rc_read_trim_device's pair cut choose it, with min_overlap and
 * max_mismatch_pct over the bases as given; with no accepted offset the pair is UNMERGED: merged_len = 0 and d = v = m = 0 in its
 * row.  The merged read has F = d* + Lb bases (the pair cut's fragment length); position p is covered by a when p < La and by r,
 * at r[p - d*], when p >= d*; what lies outside -- r[0 .. -d* - 1] for d* < 0, a[F ..] for F < La -- is read-through and is
 * dropped.  Per position (rc_merge.h, integer arithmetic), a base valid when it is upper-case ACGT, p(Q) = max(0, Q - qual_base):
 *   covered by one mate       that mate's base byte (mate 2's complemented: ACGT <-> TGCA, acgt <-> tgca, every other byte as it
 *                             is) and its quality byte, verbatim
 *   both valid and equal      that base, quality qual_base + min(pa + pb, qual_cap)
 *   both valid and different  the mate with the larger phred value wins, a tie goes to mate 1; quality
 *                             qual_base + min(max(|pa - pb|, 2), qual_cap)
 *   exactly one valid         that mate's base byte and quality byte, verbatim
 *   neither valid             mate 1's two bytes, verbatim
 *   d_qual == NULL (FASTA)    a disagreement keeps mate 1's base and counts as a tie; no quality arena is written
 * A mate has at most 1023 bases; a merged read may have up to La + Lb - min_overlap <= 2045.  Of a read longer than 1023 bases
 * rc_read_trim_device and rc_mate_overlap_device look only at the first 1023; the entry points that stage reads in the probe tile
 * (rc_read_depth_device, rc_read_screen_device) take it as no read: four zeros; rc_weak_profile_device, whose reduce walks a read
 * of any length, profiles all of it; rc_trust_profile_device counts its first windows; rc_correct_device refuses the batch.  Not in scope: merging inside rcorrector, a slot-transport registration,
 * a compacted trimmed arena, indel-tolerant overlap, posterior-probability quality models.  No byte parity with FLASH, PEAR or
 * fastp is claimed.  No reference counterpart. */
#define RC_MERGE_LEN_BINS 2048
typedef struct { int32_t merged_len, d, v, m; } rc_read_merge;     /* 16 bytes per unit: v faced valid positions at d, m of them differ */
typedef struct { int32_t min_overlap, max_mismatch_pct, qual_base, qual_cap; } rc_merge_params;   /* defaults 30, 10, 33, 41 */
typedef struct {
    uint64_t pairs, merged, unmerged;
    uint64_t readthrough;            /* merged with d* < 0 or F < La */
    uint64_t compared, mismatches;   /* the sums of v and of m over the merged pairs */
    uint64_t took_mate1, took_mate2, ties;   /* the disagreements by the mate whose base was kept: their sum is `mismatches` */
    uint64_t len_hist[RC_MERGE_LEN_BINS];    /* [merged_len], every pair: bin 0 holds the unmerged ones */
} rc_merge_tally;
/* The pairs of an arena in HBM (read r the NUL-terminated string at d_off[r] of d_seq, and of d_qual -- may be NULL -- its
 * quality bytes; d_off has n_reads + 1 entries) in mode 1 (read u with read n_reads / 2 + u) or 2 (reads 2u and 2u + 1), units =
 * n_reads / 2 of them.  d_rows[u] = the rc_read_merge of unit u.  The result is a NEW, compact arena: d_moff has units + 1
 * entries, unit u's merged read is the NUL-terminated string at d_moff[u] of d_mseq, an unmerged unit an empty string, and
 * d_moff[units] is the arena's size; d_mqual (may be NULL; must be NULL if d_qual is) gets the quality bytes at the same
 * offsets.  d_mseq / d_mqual / d_moff with units reads is an arena every per-read entry point accepts as it is in mode 0.
 * Output size: a merged unit takes F + 1 <= La + Lb + 2 - min_overlap bytes, an unmerged one 1 byte, and the two mates took
 * La + Lb + 2 bytes of the input: out_cap, the bytes d_mseq (and d_mqual) can hold, must be >= nbytes, and that is always
 * enough.  No byte at or behind d_moff[units] is written, and nothing is read from the output arenas.  d_tally (may be NULL): an
 * rc_merge_tally in HBM that the call ADDS to -- the caller zeroes it.  Three steps on the context's stream, asynchronous
 * (rc_sync() to wait): a plan kernel (the offset scan: rows and lengths), an exclusive scan of the lengths, a write kernel.
 * Needs no table; neither input arena is written, both may be read in aligned 16-byte pieces up to 15 bytes in front of their
 * first and behind their last byte.  max_read_len picks the kernel instance (up to 256 bases, or up to 1023); a mate longer than
 * its instance holds is cut to that first.  n_reads == 0: RC_STATUS_OK, no launch, nothing written.  RC_STATUS_ARG (checked
 * whatever n_reads is): a mode outside 1 .. 2, an odd n_reads, params == NULL, nbytes >= 2^32, max_read_len outside 0 .. 1023,
 * min_overlap outside 1 .. 1023, max_mismatch_pct outside 0 .. 50, qual_base outside 0 .. 124, qual_cap outside 2 .. 93,
 * qual_base + qual_cap > 126, d_mqual given without d_qual, out_cap < nbytes; with n_reads > 0: d_seq, d_off, d_rows, d_mseq or
 * d_moff NULL, d_rows or d_moff off a 4-byte boundary, d_mseq or d_mqual off a 16-byte one, d_tally
 * off an 8-byte one. */
int rc_read_merge_device(rc_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, const uint32_t *d_off, uint32_t n_reads, uint64_t nbytes,
                         int32_t max_read_len, int32_t mode, const rc_merge_params *params, rc_read_merge *d_rows,
                         uint8_t *d_mseq, uint8_t *d_mqual, uint32_t *d_moff, uint64_t out_cap, rc_merge_tally *d_tally);

/* ---- run parameters (globals of main.cpp:17-30) ----------------------------------------------- */
/* replaces main.cpp:310-358 (ERROR_RATE estimation).  Uses the entries parsed by the last
 * rc_table_load_jfdump() in file order -- or, for a table that was counted here or built from
 * arrays, the table's entries in dump order (what the reference would scan if given
 * rc_table_write_jfdump's file); the probes run on the GPU, the <=100000 divisions and the sort
 * on the host in IEEE double exactly as the reference does. */
int rc_estimate_error_rate(rc_ctx *ctx, double wk, double *rate_out);
/* replaces GetBadQuality's arithmetic (main.cpp:108-127) given the two histograms gathered over
 * the first <= 1,000,000 records (first_hist[q] = #reads whose first quality char is q,
 * last_hist likewise for the last base) */
char rc_bad_quality_from_hist(const int32_t first_hist[300], const int32_t last_hist[300], int32_t total);
/* sets ERROR_RATE and badQualityThreshold (the globals of main.cpp:24-27) for subsequent corrections; also builds
 * the inverse of GetBound (ErrorCorrection.cpp:139-142) at this rate on the host -- the reference's own arithmetic,
 * ~20 ms -- and leaves it in device memory for the kernels: call it once per run, with no batch in flight */
int rc_set_run_params(rc_ctx *ctx, double error_rate, char bad_quality);

/* Quality as one bit per base.  The correction only ever compares a quality with badQualityThreshold
 * (the vetoes, ErrorCorrection.cpp:1313-1466) and tests qual[0] != 0, so a host that is bound by the
 * upload can ship bits instead of bytes: with on != 0 every quality arena handed to this context
 * (rc_batch.qual / qual2, rc_device_batch.d_qual) is a bit array over the arena, bit (p & 7) of byte
 * p >> 3 = the quality character at arena byte p is greater than the threshold -- 19 instead of 151
 * bytes per 150-base read over PCIe.  rc_pack_quality_bits() makes such an array from a byte arena
 * (nbytes = the arena's size; bits has (nbytes + 7) / 8 bytes).  FASTQ input only (the FASTA marker
 * qual[0] == 0 cannot be expressed); same results as with bytes. */
int rc_set_quality_bits(rc_ctx *ctx, int on);
void rc_pack_quality_bits(const char *qual, size_t nbytes, char bad_quality, uint8_t *bits);

/* ---- correction (ErrorCorrection.h:12-28) ------------------------------------------------------ */
/* Batch in host memory.  Replaces struct _ErrorCorrectionThreadArg + the pthread fan-out of
 * main.cpp:439-523 / the inline loop main.cpp:368-438: one call = one batch through
 * ErrorCorrection_Thread (ErrorCorrection.cpp:73-136).
 *   read i of an arena is the NUL-terminated string at seq + off[i]; off has n+1 entries and
 *   off[i+1]-off[i] = strlen+1; qual uses the same offsets.
 *   mode 0: single-end.  mode 1: paired, mate i of arena 1 pairs with mate i of arena 2
 *   (readBatch/readBatch2).  mode 2: interleaved, reads 2j and 2j+1 are mates.
 *   Outputs: seq/seq2 corrected in place; ret = ErrorCorrection()'s return value
 *   (_Read::correction), l/m/h = GetKmerInformation().  In mode 1 entries [n, 2n) of
 *   ret/l/m/h belong to arena 2. */
typedef struct {
    int mode;
    size_t n;
    char *seq;
    const char *qual;
    const uint32_t *off;
    char *seq2;
    const char *qual2;
    const uint32_t *off2;
    int32_t *ret, *l, *m, *h;
} rc_batch;
int rc_correct_batch(rc_ctx *ctx, rc_batch *b);

/* The same, asynchronous: up to RC_MAX_SLOTS batches in flight in ONE context, so that the upload
 * of batch N+1, the kernels of batch N and the download of batch N-1 overlap -- what the reference
 * gets from filling the next batch while its worker threads correct the current one
 * (main.cpp:479-516).  rc_submit(slot) starts a batch and returns; the descriptor is copied, the
 * buffers it points to must stay valid and untouched until rc_wait(slot) returns, after which they
 * hold the results (and rc_summary() includes the batch).  Slot 0 runs in the context itself; every other slot is a LANE with
 * streams, events and scratch memory of its own (created at its first use; the table, the run parameters and the kept arenas
 * are the context's, lent), so that the kernels of batches in different slots overlap on the GPU -- a batch's last waves, on
 * its slowest reads, run under the next batch's probe kernel instead of in front of it (the reference's workers pick up the
 * next read while another one is still searching: ErrorCorrection.cpp:87-90).  Batches in different slots may therefore
 * complete in any order; rc_wait(slot) is what orders a caller.  RC_SLOT_LANES=0 in the environment keeps every slot in the
 * one context (one compute stream: batches complete in submission order), and rc_set_slot_lanes() switches at run time (it
 * applies to the batches submitted after it): lanes pay where a batch's slowest reads leave the GPU idle -- small batches, error-
 * laden data: 1 M-read batches of 150-base pairs at 0.5 % errors 174 -> 223 M reads/s, at 5 % errors and k = 31 3.5 -> 9.2 M --
 * and cost a few per cent where the caller is bound elsewhere and wants its batches back one at a time (`rcorrector` starts
 * without them and turns them on when its writer starts waiting for the GPU).
 * Buffers obtained from rc_host_alloc() are page-locked: the DMA engines read and write them
 * directly; any other buffer is staged through pinned memory the slot owns (one extra copy each
 * way).  rc_correct_batch(b) == rc_submit(b, 0); rc_wait(0).  Calls on one context come from one
 * thread at a time, with one exception: rc_wait(slot) only touches its slot and may run on another
 * thread while the next rc_submit (a different slot) is issued -- how `rcorrector` keeps several
 * worker threads busy on one context. */
#define RC_MAX_SLOTS 4
int rc_set_slot_lanes(rc_ctx *ctx, int on);
/* The lanes' streams overlap only when the HIP runtime gives them hardware queues of their own: it multiplexes a process's
 * streams onto GPU_MAX_HW_QUEUES queues, four by default, and two compute streams that share one run one after the other.
 * That variable is read when the runtime starts, so it is the HOST's to set: export GPU_MAX_HW_QUEUES=16, or call
 * rc_runtime_prepare(16) -- from one thread, before any thread exists that reads the environment and before the process
 * first touches HIP (its own use included; torch counts) -- which sets it unless the process has it already.  Returns 1 if it
 * set the variable, 0 if it was set already (left alone), -1 on a bad argument.  rc_create does not touch the environment
 * (it did until round 5); a lane created while the variable is unset or below 8 prints one note on stderr (RC_QUIET=1: none).
 * No reference counterpart: the reference's workers are pthreads on one Store (main.cpp:439-523). */
int rc_runtime_prepare(int hw_queues);
int rc_submit(rc_ctx *ctx, const rc_batch *b, int slot);
int rc_wait(rc_ctx *ctx, int slot);
int rc_host_alloc(rc_ctx *ctx, size_t bytes, void **out);
int rc_host_free(rc_ctx *ctx, void *p);
/* ... or page-lock memory the caller already owns (page-aligned, whole pages) */
int rc_host_register(void *p, size_t bytes);
int rc_host_unregister(void *p);

/* The packed boundary: what SURVEY.md section 3 gives as the device boundary of a batch -- "only packed reads go down
 * and (fix list, ret, l, m, h) come back" -- for callers bound by the PCIe link (the byte path above moves 306 bytes up
 * and 167 down per 150-base read, this one about 61 and 20).  The reads of a batch are described as ONE arena of
 * `nbytes` bytes, read i the NUL-terminated string at off[i] (mode 1: the n first mates, then the n second mates;
 * off has total + 1 entries, total = n reads of mode 0 / 2 or 2 n of mode 1); the arena itself stays with the caller:
 *   bases     2 bits per arena byte, 16 per word: byte p at bits 30 - 2 (p & 15) of word p >> 4, A0 C1 G2 T3
 *             (KmerCode.h:7-89's code); NULs and letters outside ACGT are 0.  (nbytes + 15) / 16 words.
 *   exc_pos / exc_chr   the n_exc letters outside ACGT: arena position (ascending) and the letter
 *   qual_bits one bit per arena byte as rc_pack_quality_bits() makes them, or NULL: no qualities (FASTA input,
 *             Reads.h:224-266: the reference then sees qual[0] == 0)
 * rc_pack_bases() makes bases / exc_* from a byte arena (callers with several threads pack ranges that start at multiples
 * of 16 bytes side by side: range [begin, end) writes words [begin / 16, (end + 15) / 16) and its own exception list,
 * whose positions are arena positions; a range that starts inside a word keeps the bits of the positions in front of it,
 * so the second arena of a pair is packed behind the first one: seq = arena2 - bytes1, begin = bytes1).  rc_submit_packed() starts the batch, rc_wait_packed() completes it: ret / l / m / h
 * as for rc_batch, and the substitutions the correction made (ErrorCorrection.cpp:1468-1479) as n_fix pairs
 * (fix_pos[j] = arena position, fix_chr[j] = the new letter), in no particular order -- positions are distinct, so the
 * caller may apply them from several threads (rc_apply_fixes() is the loop).  fix_cap = room in the caller's arrays;
 * more fixes than that is an error (a batch of N bases never has more than N).  All arrays of the descriptor should be
 * page-locked (rc_host_alloc); others are staged through the slot's own pinned memory.
 * The results equal rc_submit()'s on the same reads: ret / l / m / h identical, arena + fixes = the corrected arena. */
typedef struct {
    int mode;
    size_t n;               /* reads per arena as in rc_batch (mode 1: pairs) */
    uint64_t nbytes;        /* bytes of the arena (mode 1: both mates' arenas together) */
    const uint32_t *off;    /* [total + 1] */
    const uint32_t *bases;  /* [(nbytes + 15) / 16] */
    const uint8_t *qual_bits; /* [(nbytes + 7) / 8] or NULL */
    const uint32_t *exc_pos;
    const uint8_t *exc_chr;
    size_t n_exc;
    int32_t *ret, *l, *m, *h; /* [total] */
    uint32_t *fix_pos;      /* [fix_cap] */
    uint8_t *fix_chr;       /* [fix_cap] */
    size_t fix_cap;
    size_t n_fix;           /* out, valid after rc_wait_packed */
} rc_packed_batch;
/* returns the number of exceptions found in [begin, end) (all of them are counted, the first exc_cap are stored) */
size_t rc_pack_bases(const char *seq, size_t begin, size_t end, uint32_t *bases, uint32_t *exc_pos, uint8_t *exc_chr, size_t exc_cap);
int rc_submit_packed(rc_ctx *ctx, rc_packed_batch *b, int slot);
int rc_wait_packed(rc_ctx *ctx, int slot);
void rc_apply_fixes(char *seq, const uint32_t *fix_pos, const uint8_t *fix_chr, size_t n_fix);

/* The packed boundary for reads that are already in HBM -- the arenas the k-mer counter kept (rc_table_count_keep; without
 * a jellyfish dump the reads have been uploaded once to be counted, run_rcorrector.pl:262-281 reads them a second time
 * for stage 3): nothing but the offsets and the quality bits goes down, the same results come back.  A batch is a byte
 * range of one kept arena (mode 0 / 2), or of two (mode 1: first mates from arena_a, second mates from arena_b); the ranges
 * hold whole NUL-terminated reads.  off / qual_bits / ret .. fix_* / n_fix as in rc_packed_batch, over the batch's own
 * arena of bytes_a + bytes_b bytes (range a, then range b); the kept arenas themselves are never modified, so a batch
 * may be submitted again. */
typedef struct {
    int mode;
    size_t n;                  /* reads per arena as in rc_batch (mode 1: pairs) */
    int arena_a, arena_b;      /* indices of kept arenas (arena_b: mode 1 only) */
    uint64_t begin_a, bytes_a; /* the batch's byte range of arena_a */
    uint64_t begin_b, bytes_b; /* ... of arena_b (mode 1), else 0 */
    const uint32_t *off;       /* [total + 1], off[total] = bytes_a + bytes_b */
    const uint8_t *qual_bits;  /* [(bytes_a + bytes_b + 7) / 8] or NULL (FASTA) */
    int32_t *ret, *l, *m, *h;  /* [total] */
    uint32_t *fix_pos;         /* [fix_cap] positions in the batch's arena */
    uint8_t *fix_chr;          /* [fix_cap] */
    size_t fix_cap;
    size_t n_fix;              /* out, valid after rc_wait_resident */
} rc_resident_batch;
int rc_submit_resident(rc_ctx *ctx, rc_resident_batch *b, int slot);
int rc_wait_resident(rc_ctx *ctx, int slot);

/* rc_correct_batch plus everything the reference prints per read under -verbose (VERBOSE,
 * ErrorCorrection.cpp:15,686-689,759-770,856-857,1088-1094,1590-1597), as data; the caller formats
 * it (rc_main.cpp does, byte for byte).  Reads are indexed like ret/l/m/h (mode 1: arena 2's reads
 * at [n, 2n)); arena bytes are arena 1's followed by arena 2's.
 *   counts_before/after[a] = GetCount of the k-mer starting at arena byte a, before / after the
 *     correction (0 where the window holds a non-ACGT letter or runs past the read);
 *   flags[r] bit 0: read r passed the screens, i.e. "Before correction" is printed;
 *   n_iter[r]: threshold iterations of read r (may exceed max_iter: only the first max_iter are
 *     recorded);  iter + (r*max_iter + i)*RC_TRACE_ITER_WORDS: iteration i = {strong trust
 *     threshold, threshold, 1 if the bitmap was reached, 0, 32 words of the "Is corresponding base
 *     strong trusted?" bitmap (bit b of word w = base 32w+b)}. */
#define RC_TRACE_ITER_WORDS 36
typedef struct {
    int32_t max_iter;
    int32_t *counts_before, *counts_after; /* [arena bytes] */
    int32_t *flags, *n_iter;               /* [reads] */
    int32_t *iter;                         /* [reads * max_iter * RC_TRACE_ITER_WORDS] */
} rc_trace;
int rc_correct_batch_traced(rc_ctx *ctx, rc_batch *b, rc_trace *t);

/* Batch already resident in HBM (asynchronous on the context's stream; rc_sync() to wait).
 * In mode 1 the arena holds the n/2 first mates followed by the n/2 second mates.  max_read_len above 1023 (utils.h:7; a merged
 * arena may hold such reads) is RC_STATUS_ARG, refused before anything is launched: no read of the arena is corrected. */
typedef struct {
    int mode;
    uint32_t n_reads;
    uint64_t nbytes;        /* bytes of the arena (sum of strlen+1) */
    int32_t max_read_len;   /* longest read, bases */
    uint8_t *d_seq;         /* corrected in place */
    const uint8_t *d_qual;
    const uint32_t *d_off;  /* n_reads + 1 */
    int32_t *d_ret, *d_l, *d_m, *d_h;
} rc_device_batch;
int rc_correct_device(rc_ctx *ctx, const rc_device_batch *b);
/* replaces GetStrongTrustedThreshold (ErrorCorrection.h:26, ErrorCorrection.cpp:1482-1565) for every
 * read of an arena in HBM (asynchronous; the run parameters must be set): d_strong[r] = the
 * function's return value for read r (-1 for reads it screens out). */
int rc_strong_threshold_device(rc_ctx *ctx, const uint8_t *d_seq, const uint32_t *d_off, uint32_t n_reads,
                               uint64_t nbytes, int32_t max_read_len, int32_t *d_strong);
/* The three functions of ErrorCorrection.h:26-28 at the reference's own granularity, one NUL-terminated read per call
 * (each a batch of one: a kernel launch and two small copies -- for bindings that work read by read and for spot checks;
 * throughput lives in the batch calls above).  The table and the run parameters must be set.
 *   rc_strong_threshold_read  = GetStrongTrustedThreshold(seq, qual, kcode, kmers), ErrorCorrection.cpp:1482-1565
 *       (the function never reads qual);
 *   rc_correct_read           = ErrorCorrection(id, seq, qual, pairStrongTrustThreshold, kcode, kmers), :682-1480: seq is
 *       corrected in place, *ret = the return value; pair_strong_threshold = min of the two mates' strong thresholds, or
 *       -1 for a read without a mate (:96-106); qual == NULL stands for a FASTA record (qual[0] == 0, Reads.h:241);
 *       counted by rc_summary like any batch;
 *   rc_kmer_info_read         = GetKmerInformation(seq, kmerLength, kmers, l, m, h), :1567-1602, of the read as given.
 * Rules of all three (tests/test_per_read.py):
 *   - qual is a C string of its own length: one shorter than the read counts as padded with NULs (the bases behind it have
 *     quality 0, an empty one is a FASTA record like NULL), one longer is read up to the read's length;
 *   - a read of more than 1023 bases is RC_ERR_ARG (utils.h:7: MAX_READ_LENGTH 1024 with the NUL); seq is left as it was;
 *   - while rc_set_quality_bits is on, the calls are RC_ERR_STATE: they take quality bytes. */
int rc_strong_threshold_read(rc_ctx *ctx, const char *seq, int32_t *strong);
int rc_correct_read(rc_ctx *ctx, char *seq, const char *qual, int32_t pair_strong_threshold, int32_t *ret);
int rc_kmer_info_read(rc_ctx *ctx, const char *seq, int32_t *l, int32_t *m, int32_t *h);
/* the hash-probe kernel alone: d_counts[a] = count of the k-mer starting at arena byte a
 * (ErrorCorrection.cpp:716-723 for every read of the arena) */
int rc_probe_device(rc_ctx *ctx, const uint8_t *d_seq, uint64_t nbytes, int32_t *d_counts);
int rc_sync(rc_ctx *ctx);

/* ---- measurement ----------------------------------------------------------------------------- */
/* with profiling on, every kernel launch is bracketed by HIP events on the stream it runs on.  The events are only recorded
 * when the kernel is launched: no launch waits for the GPU, and the pairs are waited for and added up by rc_profile_get and
 * rc_sync (or when the context's small pool of pairs is full). */
int rc_profile_enable(rc_ctx *ctx, int on);
/* on = 2 additionally runs the instrumented build of the correction kernel (slower; same results),
 * which counts, over the launches since the last reset: the reads the threshold kernel could not
 * finish and handed to the correction kernel, their gather rounds (one round = up to 64 table
 * probes issued together) and the table buckets they read -- the denominators of the kernel's
 * request-rate figures. */
int rc_profile_correct_counters(rc_ctx *ctx, uint64_t *reads_listed, uint64_t *gather_rounds, uint64_t *bucket_requests);
/* d_rounds != NULL: the instrumented build (rc_profile_enable(ctx, 2)) also leaves the gather rounds of every read the
 * correction kernel processes in d_rounds[read index] (device memory, one int32 per read of the batch, zeroed by the caller:
 * reads finished before that kernel are not written) -- which reads of a batch the search works hardest on
 * (MAX_TRIAL, ErrorCorrection.cpp:7; the straggler of tools/find_straggler.py).  NULL switches it off. */
int rc_profile_read_rounds(rc_ctx *ctx, int32_t *d_rounds);
/* kernel 0 = probe, 1 = threshold, 2 = correct, 3 = isolated substitutions, 4 = weak-k-mer profile, 5 = the trust profile's
 * planes, 6 = its accumulate and column sums, 7 = per-read k-mer depth, 8 = per-read screen against a second k-mer set,
 * 9 = normalisation's unit selection; accumulated since the last reset (the call waits for the launches still in flight).
 * Where rc_correct_device runs a batch as a chunked pipeline (RC_PIPELINE_CHUNKS), kernels 0, 2 and 3 are
 * launched once per chunk on two streams and each kind is timed ONCE per call, from its first chunk's launch to the end of
 * its last: `launches` still counts arenas, and the three figures are spans that overlap in time -- their sum exceeds the
 * time of the step, and a span includes what its stream waited for. */
int rc_profile_get(rc_ctx *ctx, int kernel, double *total_ms, uint64_t *launches);
int rc_profile_reset(rc_ctx *ctx);

/* diagnostic: GetBound(c) (ErrorCorrection.cpp:139-142) exactly as the kernels evaluate it, for n
 * counts and one error rate: out_int = the implicit double->int conversion (cvttsd2si semantics),
 * out_dbl = the double itself (NaN for c < 0).  Lets a test compare the device arithmetic with the
 * host's bit for bit. */
int rc_selftest_get_bound(rc_ctx *ctx, const int32_t *c, size_t n, double error_rate, int32_t *out_int, double *out_dbl);

/* test support: how the last batch this context ran through rc_correct_device or rc_correct_batch was routed.  Waits for the
 * context's stream and copies, for each of its n reads: cls (0 = finished before the general correction kernel, else that
 * kernel's work class 1..4), cand (> 0 = the threshold kernel offered the read to the isolated-substitution kernel: the number
 * of its untrusted stretches) and runs (candidates only; low 32 bits: stretch 0 | stretch 1 << 16, next 16 bits: stretch 2, top
 * 16 bits: the number of stretches; a stretch = first k-mer | length << 8).  cls == 0 && cand == 0: finished by the threshold
 * kernel; cls == 0 && cand > 0: by the isolated-substitution kernel; cls != 0: by the general kernel.  Launches nothing.
 * RC_ERR_STATE (the text says which) when the arrays do not describe the whole batch: none has run, it failed, it ran in length tiers (a
 * read of more than 160 bases), without classification or without candidates, or n is not its number of reads. */
int rc_debug_routes(rc_ctx *ctx, uint8_t *cls_out, uint8_t *cand_out, uint64_t *runs_out, uint32_t n);
/* test support: the batches this context and its slot lanes ran as a chunked pipeline (RC_PIPELINE_CHUNKS) and the non-empty
 * chunks those launched, since the context was made; host counters, nothing is launched or waited for. */
int rc_debug_pipeline(rc_ctx *ctx, uint64_t *batches, uint64_t *chunks);

/* test support: the device side of the packed boundary alone (rc_submit_packed / rc_wait_packed without a correction), through
 * the launchers the transports use; needs no table and no run parameters.  All pointers are host memory.  Runs, on the context's
 * stream: the expansion of `packed` ((nbytes + 15) / 16 words, rc_pack_bases), the NULs of the n_reads reads of `off` (n_reads + 1
 * offsets over the arena's nbytes bytes) and the n_exc exceptions into a device arena of round16(nbytes) + RC_SELFTEST_ARENA_SLACK
 * bytes that held RC_SELFTEST_CANARY in every byte -- all of it comes back in unpacked_out --; then, with the arena's first nbytes
 * bytes replaced by `after` (what a correction would have left; the padding stays as expanded), the fix list against the packed
 * codes and the exceptions with room for `cap` entries, into device arrays of cap + RC_SELFTEST_FIX_SLACK entries that held the
 * canary in every byte: *n_fix_out = the number of fixes (all of them, as rc_packed_batch.n_fix), fix_pos_out / fix_chr_out = the
 * arrays with their slack.  Waits for the stream.  RC_ERR_ARG for null or inconsistent arguments: offsets that do not ascend from 0
 * to nbytes, an exception outside the arena. */
#define RC_SELFTEST_CANARY 0xA5
#define RC_SELFTEST_ARENA_SLACK 64
#define RC_SELFTEST_FIX_SLACK 64
int rc_selftest_transport_packed(rc_ctx *ctx, const uint32_t *packed, size_t nbytes, const uint32_t *off, uint32_t n_reads, const uint32_t *exc_pos,
                                 const uint8_t *exc_chr, uint32_t n_exc, const uint8_t *after, uint8_t *unpacked_out, uint32_t *n_fix_out, uint32_t cap,
                                 uint32_t *fix_pos_out, uint8_t *fix_chr_out);
/* test support: the fix list of the resident boundary alone (rc_submit_resident's byte comparison), through the transport's
 * launcher.  orig_a: shift_a + na + RC_SELFTEST_ARENA_SLACK host bytes that go to a 16-byte aligned device address as they are --
 * shift_a (0..15) bytes in front, the na uncorrected bytes of the first range, the slack a kept arena carries behind them; orig_b
 * likewise for the second range (NULL where nb == 0).  after: the na + nb bytes of the corrected arena, placed at an aligned
 * address.  n_fix_out, cap, fix_pos_out and fix_chr_out as above.  Waits for the stream; RC_ERR_ARG for null arguments, a shift
 * above 15 or 4 GiB and more. */
int rc_selftest_transport_bytes(rc_ctx *ctx, const uint8_t *orig_a, size_t na, uint32_t shift_a, const uint8_t *orig_b, size_t nb, uint32_t shift_b,
                                const uint8_t *after, uint32_t *n_fix_out, uint32_t cap, uint32_t *fix_pos_out, uint8_t *fix_chr_out);

/* summary counters, struct _summary main.cpp:32-36,73-79: reads and corrected bases of every batch
 * this context has corrected through any entry point (accumulated on the device; waits for the
 * context's kernels) */
int rc_summary(const rc_ctx *ctx, uint64_t *total_reads, uint64_t *total_corrections);

#ifdef __cplusplus
}
#endif
#endif
