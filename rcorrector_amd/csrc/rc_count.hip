// rc_count.hip -- exact k-mer counter in bounded memory (stages 0-2 of run_rcorrector.pl:262-281 for reads that are, or
// pass through, HBM).  `jellyfish bc` + `count --bc` exist so that the singletons of a data set -- most of its
// distinct k-mers once reads carry errors -- never occupy the counter (run_rcorrector.pl:262-273).  Here the same
// end is reached by cutting the KEY SPACE instead: the arenas handed over are kept in HBM (one byte per base:
// 100 M x 150 bp are 15 GB of 288), and finish() makes P passes over them; pass p looks only at the k-mers whose
// hash falls into slice p of P -- emit -> radix sort -> run-length encode -> keep count >= min_count -- so that no
// more than 1/P of the k-mer occurrences is ever in flight, whatever share of them are singletons.  A histogram
// pass sizes the slices; P follows from the memory the passes may use (RC_COUNT_MEM_MB, default 24 GiB).  The result
// is what `jellyfish count -C` + `dump -L 2` hands to the reference: every canonical k-mer with its exact count.
// Three finishes are made of the steps below: rc_count_finish (the table), rc_recount_finish_session (the census of a recount
// session, rc_table.hip: k_census) and rc_count_finish_sharded (reads spread over several GPUs).  None is on the correction hot path.
#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "rc_internal.h"
#include "rc_device.h"

__global__ void k_u32_to_i32_clamped(const uint32_t *in, int32_t *out, size_t n)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = in[i] > 0x7fffffffu ? 0x7fffffff : (int32_t)in[i];
}

__device__ __forceinline__ uint32_t rc_count_slice(uint64_t key, uint32_t P)
{
    return (uint32_t)(((uint64_t)rc_hash(key ^ 0x9E3779B97F4A7C15ull) * P) >> 32);
}

// MODE 0: hist[slice] += valid k-mers of the tile; MODE 1: the canonical codes of slice `p` are appended to out.  k_probe's
// tile (rc_device.h: rc_tile_stage) without the NUL plane; seq is 16-byte aligned.
template <int MODE>
__global__ __launch_bounds__(RC_PROBE_THREADS) void k_count_scan(const uint8_t *__restrict__ seq, size_t nbytes, int k, uint32_t P, uint32_t p,
                                                                 unsigned long long *__restrict__ hist, uint64_t *__restrict__ out,
                                                                 unsigned long long *__restrict__ cursor)
{
    __shared__ uint32_t s_code[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_inv[RC_PROBE_TILE / 16 + 4];
    __shared__ uint32_t s_hist[64];
    const size_t tile0 = (size_t)blockIdx.x * RC_PROBE_TILE;
    const int t = threadIdx.x;
    if (MODE == 0 && t < 64) s_hist[t] = 0;
    rc_tile_stage<false>(seq, 0, nbytes, tile0, s_code, s_inv, nullptr);  // no NUL plane: a NUL is also "not ACGT"
    __syncthreads();
    const uint32_t *m_inv = reinterpret_cast<const uint32_t *>(s_inv);
    // the canonical code of the window at tile position a, if it is a k-mer of a read, and its slice
    auto window = [&](int a, uint64_t &key, uint32_t &sl) -> bool {
        const size_t g = tile0 + (size_t)a;
        if (g + (size_t)k > nbytes) return false;
        const rc_tile_win w = rc_tile_window<false>(s_code, m_inv, nullptr, a, k);
        if (w.bad) return false;
        key = rc_canonical(w.code, k);
        sl = rc_count_slice(key, P);
        return true;
    };
    constexpr int ITER = RC_PROBE_TILE / RC_PROBE_THREADS, WAVES = RC_PROBE_THREADS / 64;
    if (MODE == 0) {
        for (int it = 0; it < ITER; ++it) {
            uint64_t key;
            uint32_t sl;
            if (window(it * RC_PROBE_THREADS + t, key, sl)) atomicAdd(&s_hist[sl & 63u], 1u);  // (P <= 64)
        }
        __syncthreads();
        if (t < 64 && s_hist[t]) atomicAdd(hist + t, (unsigned long long)s_hist[t]);
        return;
    }
    // MODE 1: ONE atomic on the output cursor per workgroup (one word sustains ~90 atomics per microsecond; a wave-level
    // reservation is 60 times as many): count the keys of slice p per (iteration, wave), reserve, then write
    __shared__ uint32_t s_n[ITER * WAVES + 1];
    __shared__ unsigned long long s_base;
    const int wv = t >> 6, lane = t & 63;
    for (int it = 0; it < ITER; ++it) {
        uint64_t key;
        uint32_t sl;
        const bool take = window(it * RC_PROBE_THREADS + t, key, sl) && sl == p;
        const unsigned long long m = __ballot(take);
        if (lane == 0) s_n[it * WAVES + wv] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (t == 0) {
        uint32_t run = 0;
        for (int i = 0; i < ITER * WAVES; ++i) {
            const uint32_t c = s_n[i];
            s_n[i] = run;
            run += c;
        }
        s_base = run ? atomicAdd(cursor, (unsigned long long)run) : 0ull;
    }
    __syncthreads();
    const unsigned long long base = s_base;
    for (int it = 0; it < ITER; ++it) {
        uint64_t key = 0;
        uint32_t sl;
        const bool take = window(it * RC_PROBE_THREADS + t, key, sl) && sl == p;
        const unsigned long long m = __ballot(take);
        if (take) out[base + s_n[it * WAVES + wv] + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull))] = key;
    }
}

__global__ void k_flag_keep(const uint64_t *__restrict__ uniq, const uint32_t *__restrict__ cnt, size_t n, int min_count,
                            uint8_t *__restrict__ keep)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keep[i] = cnt[i] >= (uint32_t)min_count ? 1 : 0;
}

static double rc_now() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// ---- arena sets (rc_internal.h) -----------------------------------------------------------------------------------------
void rc_arena_set::release()
{
    for (auto &c : chunks)
        if (c.p) (void)hipFree(c.p);
    chunks.clear();
    arenas.clear();
    chunk_used = 0;
    total = 0;
}

// an arena's place in the chunks (behind the last one in the current chunk, 256-byte aligned with 64 bytes of slack, or
// a new chunk) and its copy there on stream `st`, complete when this returns: the caller's buffer is its own again
int rc_arena_set::keep(rc_ctx *ctx, const uint8_t *seq, size_t nbytes, bool from_device, hipStream_t st, const char *what)
{
    const size_t need = (nbytes + 64 + 255) & ~(size_t)255, chunk_bytes = (size_t)2 << 30;
    if (chunks.empty() || chunk_used + need > chunks.back().bytes) {
        rc_dbuf c;
        c.bytes = need > chunk_bytes ? need : chunk_bytes;
        RC_CHECK_HIP(ctx, hipMalloc(&c.p, c.bytes));
        chunks.push_back(c);
        chunk_used = 0;
    }
    rc_dbuf a;
    a.p = (char *)chunks.back().p + chunk_used;
    a.bytes = nbytes;
    hipError_t e = hipMemcpyAsync(a.p, seq, nbytes, from_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);  // (the caller's buffer is its own again when this returns)
    if (e != hipSuccess) {
        rc_set_error(ctx, "%s: copy failed: %s", what, hipGetErrorString(e));
        return RC_ERR_HIP;
    }
    chunk_used += need;
    arenas.push_back(a);
    total += nbytes;
    return RC_OK;
}

// ---- the counting session ----------------------------------------------------------------------------------------------
int rc_count_begin(rc_ctx *ctx)
{
    if (ctx->rec_active) {
        rc_set_error(ctx, "count_begin: a recount session is open (rc_recount_finish it first)");
        return RC_ERR_STATE;
    }
    ctx->cnt.release();
    ctx->kept.release();
    ctx->spec_counted.clear();
    ctx->cnt_active = true;
    return RC_OK;
}

// what a session may keep in HBM
static size_t rc_count_retain_cap()
{
    size_t cap = (size_t)128 << 30;
    if (const char *e = getenv("RC_COUNT_RETAIN_MB")) cap = (size_t)atoll(e) << 20;
    return cap;
}

// keeps a copy of the arena in HBM (from_device: d_seq is device memory, else host memory)
int rc_count_add(rc_ctx *ctx, const uint8_t *seq, size_t nbytes, bool from_device)
{
    if (!ctx->cnt_active) {
        rc_set_error(ctx, "count_add: call rc_table_count_begin first");
        return RC_ERR_STATE;
    }
    if (nbytes == 0) return RC_OK;
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "count: an arena must be below 2^32 bytes (add it in pieces)");
        return RC_ERR_ARG;
    }
    const size_t cap = rc_count_retain_cap();
    if (ctx->cnt.total + nbytes > cap) {
        rc_set_error(ctx, "count: %zu MB of reads exceed what the k-mer counter keeps in HBM (%zu MB, RC_COUNT_RETAIN_MB): count them with "
                          "jellyfish and pass the dump (-c)", (ctx->cnt.total + nbytes) >> 20, cap >> 20);
        return RC_ERR_NOMEM;
    }
    return ctx->cnt.keep(ctx, seq, nbytes, from_device, ctx->stream, "count_add");
}

// the end of a counting session: its arenas become the kept ones (rc_submit_resident corrects the reads where they lie) or go
static void rc_count_end(rc_ctx *ctx, bool keep)
{
    ctx->cnt_active = false;
    if (keep) ctx->cnt.move_to(ctx->kept);
    ctx->cnt.release();
}

// ---- the steps every finish is made of ----------------------------------------------------------------------------------
// passes: a pass holds, per k-mer occurrence of its slice, the key (8 B), its sorted copy (8 B), the sort's scratch
// (~8 B) and the run-length output (8 + 4 + 1 B).  The slices, and with them the order of the table's entries, follow from
// P alone: the sharded finish builds the table one GPU would because it plans here too.
static uint32_t rc_count_plan(size_t total_bytes)
{
    size_t mem = (size_t)24 << 30;
    if (const char *e = getenv("RC_COUNT_MEM_MB")) mem = (size_t)atoll(e) << 20;
    const double per_occ = 40.0;
    uint32_t P = (uint32_t)((double)total_bytes * per_occ * 1.15 / (double)mem) + 1;
    if (P > 64) P = 64;
    return P;
}

// k_count_scan over a set of arenas, queued on `st` (MODE 0: hist; MODE 1: slice p's codes to out, through cursor)
template <int MODE>
static void rc_count_scan(const std::vector<rc_dbuf> &arenas, hipStream_t st, int k, uint32_t P, uint32_t p, unsigned long long *hist, uint64_t *out,
                          unsigned long long *cursor)
{
    for (const auto &a : arenas) {
        const unsigned G = (unsigned)((a.bytes + RC_PROBE_TILE - 1) / RC_PROBE_TILE);
        if (MODE == 0)
            hipLaunchKernelGGL(k_count_scan<0>, dim3(G), dim3(RC_PROBE_THREADS), 0, st, (const uint8_t *)a.p, a.bytes, k, P, p, hist, out, cursor);
        else
            hipLaunchKernelGGL(k_count_scan<1>, dim3(G), dim3(RC_PROBE_THREADS), 0, st, (const uint8_t *)a.p, a.bytes, k, P, p, hist, out, cursor);
    }
}

// rocPRIM's select of the flagged codes (tmp == nullptr: the size query)
static hipError_t rc_select_codes(void *tmp, size_t &tmp_bytes, const uint64_t *in, const uint8_t *flags, uint64_t *out, size_t *d_n, size_t n, hipStream_t st)
{
    return rocprim::select(tmp, tmp_bytes, in, flags, out, d_n, n, st);
}

// One allocation holds the scratch of slices of up to max_slice occurrences: the emitted codes (keys; after the reduce step
// the distinct codes, ascending), their sorted copy (keys_s; after the select step the kept codes), the run lengths (cnt), the
// keep flags, one size_t on the device and rocPRIM's scratch, enough for a sort, a run-length encode or a select.  (Round 3
// allocated per pass and concatenated at the end: some forty hipMalloc / hipFree calls, each a round trip through the kernel
// driver -- 0.1 s on a quiet host, 0.5 s and more on a busy one, against 0.2 s for the counting itself.)
struct rc_slice_scratch {
    rc_dev_tmp pool;
    uint64_t *keys = nullptr, *keys_s = nullptr;
    uint32_t *cnt = nullptr;
    uint8_t *keep = nullptr;
    size_t *d_runs = nullptr;
    void *tmp = nullptr;
    size_t tmp_bytes = 0;
    int end_bit = 64;  // of the sort: the codes have 2 k bits

    int alloc(rc_ctx *ctx, size_t max_slice, int k, hipStream_t st)
    {
        end_bit = 2 * k > 64 ? 64 : 2 * k;
        size_t ts_sort = 0, ts_rle = 0, ts_sel = 0;
        RC_CHECK_HIP(ctx, rocprim::radix_sort_keys(nullptr, ts_sort, (uint64_t *)nullptr, (uint64_t *)nullptr, max_slice, 0, end_bit, st));
        RC_CHECK_HIP(ctx, rocprim::run_length_encode(nullptr, ts_rle, (uint64_t *)nullptr, (unsigned int)max_slice, (uint64_t *)nullptr, (uint32_t *)nullptr,
                                                     (size_t *)nullptr, st));
        RC_CHECK_HIP(ctx, rc_select_codes(nullptr, ts_sel, nullptr, nullptr, nullptr, nullptr, max_slice, st));
        tmp_bytes = std::max(ts_sort, std::max(ts_rle, ts_sel));
        auto up = [](size_t x) { return (x + 255) & ~(size_t)255; };
        const size_t o_keys_s = up(max_slice * 8), o_cnt = o_keys_s + up(max_slice * 8), o_keep = o_cnt + up(max_slice * 4), o_runs = o_keep + up(max_slice),
                     o_tmp = o_runs + 256;
        RC_CHECK_HIP(ctx, pool.alloc(o_tmp + up(tmp_bytes)));
        char *p = pool.as<char>();
        keys = (uint64_t *)p;
        keys_s = (uint64_t *)(p + o_keys_s);
        cnt = (uint32_t *)(p + o_cnt);
        keep = (uint8_t *)(p + o_keep);
        d_runs = (size_t *)(p + o_runs);
        tmp = p + o_tmp;
        return RC_OK;
    }
};

// The three steps of a slice only queue work on `st`, a stream of the scratch's device (the current one); their result is in a
// host word once the stream has been waited for (the sharded finish runs several owners side by side).  Errors go to `ctx`.
// Reduce: the m codes in S.keys -> sorted (S.keys_s) -> run-length encoded: *runs distinct codes in S.keys, ascending, with their
// counts in S.cnt.  t_sort (RC_COUNT_TIMING): the exception, waits for the sort and adds its time.
static int rc_slice_reduce(rc_ctx *ctx, rc_slice_scratch &S, size_t m, hipStream_t st, size_t *runs, double *t_sort)
{
    const double tp = rc_now();
    size_t t1 = S.tmp_bytes;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_keys(S.tmp, t1, S.keys, S.keys_s, m, 0, S.end_bit, st));
    if (t_sort) {
        RC_CHECK_HIP(ctx, hipStreamSynchronize(st));
        *t_sort += rc_now() - tp;
    }
    t1 = S.tmp_bytes;
    RC_CHECK_HIP(ctx, rocprim::run_length_encode(S.tmp, t1, S.keys_s, (unsigned int)m, S.keys, S.cnt, S.d_runs, st));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(runs, S.d_runs, sizeof(size_t), hipMemcpyDeviceToHost, st));
    return RC_OK;
}

// Select: the counts of a reduced slice into the spectrum d_spec (rc_table_count_spectrum, before the min_count filter; spec_bin
// 0: none), then the codes seen at least min_count times: *nsel of them in S.keys_s (free again after the sort)
static int rc_slice_select(rc_ctx *ctx, rc_slice_scratch &S, size_t runs, int min_count, uint32_t spec_bin, unsigned long long *d_spec, hipStream_t st,
                           size_t *nsel)
{
    if (spec_bin) {
        const int rs = rc_launch_spectrum_counts(ctx, st, S.cnt, runs, spec_bin, d_spec);
        if (rs) return rs;
    }
    hipLaunchKernelGGL(k_flag_keep, dim3((unsigned)((runs + 255) / 256)), dim3(256), 0, st, S.keys, S.cnt, runs, min_count, S.keep);
    size_t t1 = S.tmp_bytes;
    RC_CHECK_HIP(ctx, rc_select_codes(S.tmp, t1, S.keys, S.keep, S.keys_s, S.d_runs, runs, st));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(nsel, S.d_runs, sizeof(size_t), hipMemcpyDeviceToHost, st));
    return RC_OK;
}

// The kept entries of all slices go straight into two arrays a table can be built from.  Their number is known only at the
// end: the arrays are sized by their owner's estimate when the first slice keeps anything, and regrown in the rare case a
// later slice does not fit.
struct rc_kept_arrays {
    rc_dev_tmp k, c;  // canonical codes, counts
    size_t n = 0, cap = 0;
};

// Append: the nsel codes a select step left in S.keys_s behind the K.n entries there are; their counts go through a second
// select into the same buffer and from there, clamped to int32, to their place.  `want`: the capacity to grow to if they do not
// fit (the wait for the copy of what is there is the one in this step).  t_alloc: the time that took is added to it.
static int rc_kept_append(rc_ctx *ctx, rc_kept_arrays &K, rc_slice_scratch &S, size_t runs, size_t nsel, size_t want, hipStream_t st, double *t_alloc)
{
    if (K.n + nsel > K.cap) {
        const double ta = rc_now();
        static const bool tight = getenv("RC_COUNT_TIGHT") != nullptr;  // tests: no slack, every slice regrows the arrays
        if (want < K.n + nsel || tight) want = K.n + nsel;
        rc_dev_tmp nk, nc;
        RC_CHECK_HIP(ctx, nk.alloc((want + 1) * 8));
        RC_CHECK_HIP(ctx, nc.alloc((want + 1) * 4));
        if (K.n) {
            RC_CHECK_HIP(ctx, hipMemcpyAsync(nk.p, K.k.p, K.n * 8, hipMemcpyDeviceToDevice, st));
            RC_CHECK_HIP(ctx, hipMemcpyAsync(nc.p, K.c.p, K.n * 4, hipMemcpyDeviceToDevice, st));
            RC_CHECK_HIP(ctx, hipStreamSynchronize(st));
        }
        std::swap(nk.p, K.k.p);
        std::swap(nc.p, K.c.p);
        K.cap = want;
        if (t_alloc) *t_alloc += rc_now() - ta;
    }
    RC_CHECK_HIP(ctx, hipMemcpyAsync(K.k.as<uint64_t>() + K.n, S.keys_s, nsel * 8, hipMemcpyDeviceToDevice, st));
    uint32_t *selc = reinterpret_cast<uint32_t *>(S.keys_s);  // (keys_s was copied out: the stream orders the reuse)
    size_t t1 = S.tmp_bytes;
    RC_CHECK_HIP(ctx, rocprim::select(S.tmp, t1, S.cnt, S.keep, selc, S.d_runs, runs, st));
    hipLaunchKernelGGL(k_u32_to_i32_clamped, dim3((unsigned)((nsel + 255) / 256)), dim3(256), 0, st, selc, K.c.as<int32_t>() + K.n, nsel);
    RC_CHECK_HIP(ctx, hipGetLastError());
    K.n += nsel;
    return RC_OK;
}

// ---- the pass loop of the one-GPU finishes (rc_count_finish: the table; rc_recount_finish_session: the census) ----------------
// One key slice, reduced, as a pass hands it to its consumer: `runs` distinct canonical codes in S.keys (ascending) with their
// counts in S.cnt.  The rest of the scratch is free for the consumer; all of it is overwritten by the next pass, which the
// stream orders behind what the consumer queued.
struct rc_count_pass {
    uint32_t p, P;
    const unsigned long long *hist;  // k-mer occurrences per slice
    unsigned long long occ_total;
    size_t runs;
    rc_slice_scratch &S;
};
// where the passes spent their time (sort / rle: with RC_COUNT_TIMING's extra synchronisations)
struct rc_count_times {
    uint32_t P = 0;
    double alloc = 0, emit = 0, sort = 0, rle = 0;
};

// histogram -> P passes over the arenas: emit slice p's canonical codes -> radix sort -> run-length encode -> consume(pass).
// Returns with the stream drained.
template <class F>
static int rc_count_passes(rc_ctx *ctx, const rc_arena_set &A, bool timing, rc_count_times &T, F &&consume)
{
    const int k = ctx->k;
    const uint32_t P = rc_count_plan(A.total);
    T.P = P;
    rc_dev_tmp b_hist, b_cursor;
    RC_CHECK_HIP(ctx, b_hist.alloc(64 * 8));
    RC_CHECK_HIP(ctx, b_cursor.alloc(8));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_hist.p, 0, 64 * 8, ctx->stream));
    rc_count_scan<0>(A.arenas, ctx->stream, k, P, 0u, b_hist.as<unsigned long long>(), nullptr, nullptr);
    RC_CHECK_HIP(ctx, hipGetLastError());
    unsigned long long hist[64];
    RC_CHECK_HIP(ctx, hipMemcpyAsync(hist, b_hist.p, sizeof hist, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    size_t max_slice = 0;
    for (uint32_t p = 0; p < P; ++p) max_slice = std::max(max_slice, (size_t)hist[p]);
    if (max_slice >= (1ull << 32)) {
        rc_set_error(ctx, "count: a pass of %zu k-mer occurrences exceeds 2^32 (lower RC_COUNT_MEM_MB for more passes)", max_slice);
        return RC_ERR_ARG;
    }
    if (max_slice == 0) return RC_OK;
    rc_slice_scratch S;
    const double ta0 = rc_now();
    const int ra = S.alloc(ctx, max_slice, k, ctx->stream);
    if (ra) return ra;
    T.alloc += rc_now() - ta0;
    unsigned long long occ_total = 0;
    for (uint32_t p = 0; p < P; ++p) occ_total += hist[p];
    for (uint32_t p = 0; p < P; ++p) {
        const size_t m = (size_t)hist[p];
        if (m == 0) continue;
        RC_CHECK_HIP(ctx, hipMemsetAsync(b_cursor.p, 0, 8, ctx->stream));
        rc_count_scan<1>(A.arenas, ctx->stream, k, P, p, nullptr, S.keys, b_cursor.as<unsigned long long>());
        RC_CHECK_HIP(ctx, hipGetLastError());
        double tp = rc_now();
        if (timing) {
            RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            T.emit += rc_now() - tp;
            tp = rc_now();
        }
        const double sort0 = T.sort;
        size_t runs = 0;
        const int rr = rc_slice_reduce(ctx, S, m, ctx->stream, &runs, timing ? &T.sort : nullptr);
        if (rr) return rr;
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        T.rle += rc_now() - tp - (T.sort - sort0);
        if (runs == 0) continue;
        const rc_count_pass pass = {p, P, hist, occ_total, runs, S};
        const int rc = consume(pass);
        if (rc) return rc;
    }
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

// the table from the kept entries, on ctx; the codes stay for rc_estimate_error_rate (rc_table_release frees them)
static int rc_count_build(rc_ctx *ctx, rc_kept_arrays &K, int64_t *n_kmers)
{
    const int rc = rc_build_table_from_device_pairs(ctx, K.k.as<uint64_t>(), K.c.as<int32_t>(), K.n);
    if (rc == RC_OK && K.n) {
        ctx->counted_codes = K.k.p;
        ctx->counted_n = K.n;
        K.k.p = nullptr;
    }
    if (n_kmers) *n_kmers = (int64_t)K.n;
    return rc;
}

int rc_count_finish(rc_ctx *ctx, int min_count, int64_t *n_kmers)
{
    if (!ctx->cnt_active) {
        rc_set_error(ctx, "count_finish: call rc_table_count_begin first");
        return RC_ERR_STATE;
    }
    ctx->cnt_active = false;
    // RC_COUNT_TIMING=1 (dev): where finish() spends its time, on stderr
    static const bool timing = getenv("RC_COUNT_TIMING") != nullptr;
    const double t_begin = rc_now();
    rc_count_times T;
    double t_sel = 0;  // (with the synchronisations the selection needs anyway)
    struct release_on_exit {
        rc_ctx *c;
        ~release_on_exit() { c->cnt.release(); }  // (an error leaves nothing behind; success with cnt_keep has moved the arenas out)
    } guard{ctx};
    // rc_table_count_spectrum: every slice's run-length counts, before the min_count filter, into one device array
    const uint32_t spec_bin = ctx->spec_arm;
    rc_dev_tmp b_spec;
    if (spec_bin) {
        RC_CHECK_HIP(ctx, b_spec.alloc(((size_t)spec_bin + 5) * 8));
        RC_CHECK_HIP(ctx, hipMemsetAsync(b_spec.p, 0, ((size_t)spec_bin + 5) * 8, ctx->stream));
    }
    rc_kept_arrays K;
    const int prc = rc_count_passes(ctx, ctx->cnt, timing, T, [&](const rc_count_pass &s) -> int {
        const double tp = rc_now();
        size_t nsel = 0;
        const int rs = rc_slice_select(ctx, s.S, s.runs, min_count, spec_bin, b_spec.as<unsigned long long>(), ctx->stream, &nsel);
        if (rs) return rs;
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        t_sel += rc_now() - tp;
        if (nsel == 0) return RC_OK;
        // the arrays' size: what the passes so far kept of their occurrences, applied to all occurrences, + 15 % (+ 50 % when
        // that has already proved too little once)
        unsigned long long seen = 0;
        for (uint32_t q = 0; q <= s.p; ++q) seen += s.hist[q];
        const double per_occ_kept = (double)(K.n + nsel) / (double)(seen ? seen : 1);
        const size_t want = (size_t)(per_occ_kept * (double)s.occ_total * (K.cap ? 1.5 : 1.15)) + ((size_t)1 << 20);
        return rc_kept_append(ctx, K, s.S, s.runs, nsel, want, ctx->stream, &T.alloc);
    });
    if (prc) return prc;
    if (spec_bin) {
        std::vector<uint64_t> f((size_t)spec_bin + 5);
        RC_CHECK_HIP(ctx, hipMemcpyAsync(f.data(), b_spec.p, f.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        ctx->spec_counted = std::move(f);
    }
    if (!K.k.p) {  // nothing kept: the build still wants its two arrays
        RC_CHECK_HIP(ctx, K.k.alloc(8));
        RC_CHECK_HIP(ctx, K.c.alloc(4));
    }
    const double t_passes = rc_now();
    rc_count_end(ctx, ctx->cnt_keep);  // the reads are no longer needed here: their memory goes to the table build (or they stay for rc_submit_resident)
    const double t_concat = rc_now();
    const int rc = rc_count_build(ctx, K, n_kmers);
    if (timing)
        fprintf(stderr, "[rc count timing] finish %.3f s: histogram + %u passes %.3f (emit %.3f, sort %.3f, run lengths %.3f, select %.3f, hipMalloc %.3f), reads released %.3f, table build %.3f\n",
                rc_now() - t_begin, T.P, t_passes - t_begin, T.emit, T.sort, T.rle, t_sel, T.alloc, t_concat - t_passes, rc_now() - t_concat);
    if (rc != RC_OK) ctx->kept.release();
    return rc;
}

// ends a counting session without counting: the arenas it was given become kept arenas (rc_submit_resident), no table is built
int rc_count_park(rc_ctx *ctx)
{
    if (!ctx->cnt_active) {
        rc_set_error(ctx, "count_park: call rc_table_count_begin first");
        return RC_ERR_STATE;
    }
    rc_count_end(ctx, true);
    return RC_OK;
}

int rc_count_reads(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, int min_count, int64_t *n_kmers)
{
    if (nbytes == 0 || nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "count: arena must be 1..2^32-1 bytes");
        return RC_ERR_ARG;
    }
    int rc = rc_count_begin(ctx);
    if (rc == RC_OK) rc = rc_count_add(ctx, d_seq, nbytes, true);
    if (rc == RC_OK) rc = rc_count_finish(ctx, min_count, n_kmers);
    return rc;
}

// ---- recount session (include/rcorrector_amd.h: rc_recount_begin): a second, read-only use of the counter ------------------
// The session's arenas live in chunks of their own (rc_ctx::rec), so neither the counter's session nor the kept arenas are
// touched; finish() runs the pass loop over them and hands every slice to the census kernel (rc_table.hip) instead of the
// table build.
void rc_recount_release(rc_ctx *ctx)
{
    ctx->rec.release();
    ctx->rec_active = false;
}

int rc_recount_begin_session(rc_ctx *ctx, uint32_t max_bin)
{
    rc_recount_release(ctx);  // (a session that was never finished)
    ctx->rec_bin = max_bin;
    ctx->rec_active = true;
    return RC_OK;
}

// a copy of the arena into the session's chunks, on stream `st` of the session's device (a slot lane's for the batches it ran)
int rc_recount_append(rc_ctx *ctx, const uint8_t *seq, size_t nbytes, bool from_device, hipStream_t st)
{
    if (nbytes == 0) return RC_OK;
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "recount: an arena must be below 2^32 bytes (add it in pieces)");
        return RC_ERR_ARG;
    }
    std::lock_guard<std::mutex> lock(ctx->rec_mutex);  // (batches of several slots may complete on threads of their own)
    const size_t cap = rc_count_retain_cap();
    int rc = RC_OK;
    if (ctx->rec.total + nbytes > cap) {
        rc_set_error(ctx, "recount: %zu MB of reads exceed what a counting session keeps in HBM (%zu MB, RC_COUNT_RETAIN_MB)", (ctx->rec.total + nbytes) >> 20, cap >> 20);
        rc = RC_ERR_NOMEM;
    } else {
        rc = ctx->rec.keep(ctx, seq, nbytes, from_device, st, "recount_add");
    }
    if (rc) rc_recount_release(ctx);  // an error ends the session and leaves nothing allocated
    return rc;
}

// out: freq[rec_bin + 1], then distinct, total, unique, max_count, absent_distinct, absent_total
int rc_recount_finish_session(rc_ctx *ctx, std::vector<uint64_t> *out)
{
    static const bool timing = getenv("RC_COUNT_TIMING") != nullptr;
    const double t_begin = rc_now();
    struct release_on_exit {
        rc_ctx *c;
        ~release_on_exit() { rc_recount_release(c); }  // (success or error: the session is over, nothing stays allocated)
    } guard{ctx};
    const uint32_t max_bin = ctx->rec_bin;
    const size_t words = (size_t)max_bin + 7;
    rc_dev_tmp b_out;
    RC_CHECK_HIP(ctx, b_out.alloc(words * 8));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_out.p, 0, words * 8, ctx->stream));
    rc_count_times T;
    double t_census = 0;
    const int prc = rc_count_passes(ctx, ctx->rec, timing, T, [&](const rc_count_pass &s) -> int {
        const double tp = rc_now();
        const int rc = rc_launch_census(ctx, ctx->stream, s.S.keys, s.S.cnt, s.runs, max_bin, b_out.as<unsigned long long>());
        if (rc == RC_OK && timing) {
            RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
            t_census += rc_now() - tp;
        }
        return rc;
    });
    if (prc) return prc;
    out->assign(words, 0);
    RC_CHECK_HIP(ctx, hipMemcpyAsync(out->data(), b_out.p, words * 8, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (timing)
        fprintf(stderr, "[rc recount timing] finish %.3f s: histogram + %u passes over %zu MB (emit %.3f, sort %.3f, run lengths %.3f, census %.3f, hipMalloc %.3f)\n",
                rc_now() - t_begin, T.P, ctx->rec.total >> 20, T.emit, T.sort, T.rle, t_census, T.alloc);
    return RC_OK;
}

// ---- the counter over several GPUs ---------------------------------------------------------------------------------------
// rc_count_finish for reads that are spread over n contexts, one per GPU (`rcorrector -gpus N` in one pass: a batch's bases
// are uploaded to the GPU that will correct it, and nowhere else).  The key space is cut into the P slices one GPU would
// use; slice p belongs to GPU p % n: every GPU emits that slice's keys from its own arenas and sends them to the owner,
// which sorts, run-length encodes and selects them -- so each GPU scans a 1 / n share of the reads P times and sorts a
// 1 / n share of the keys, and every occurrence crosses xGMI once.  The kept entries are put end to end in slice order on
// cs[0], where the table is built: the same entries in the same order as rc_count_finish on one GPU holding all the reads
// (the ERROR_RATE sample and the dump depend on that order).  cs[0]'s min_count / keep / spectrum settings apply to all, and
// every error is reported on it.
int rc_count_finish_sharded(rc_ctx **cs, int n, int min_count, int64_t *n_kmers)
{
    rc_ctx *c0 = cs[0];
    for (int g = 0; g < n; ++g) {
        if (!cs[g] || !cs[g]->cnt_active) {
            rc_set_error(c0, "count_finish_sharded: every context needs an open counting session (rc_table_count_begin)");
            return RC_ERR_STATE;
        }
        if (cs[g]->k != c0->k) {
            rc_set_error(c0, "count_finish_sharded: contexts must have the same k");
            return RC_ERR_ARG;
        }
        for (int h = 0; h < g; ++h)
            if (cs[h] == cs[g]) {
                rc_set_error(c0, "count_finish_sharded: a context is listed twice");
                return RC_ERR_ARG;
            }
    }
    struct release_all {
        rc_ctx **cs;
        int n;
        ~release_all()
        {
            for (int g = 0; g < n; ++g) {
                (void)hipSetDevice(cs[g]->device);
                rc_count_end(cs[g], false);  // (success with cnt_keep has moved the arenas out)
            }
            (void)hipSetDevice(cs[0]->device);
        }
    } guard{cs, n};
    const int k = c0->k;
    size_t total = 0;
    for (int g = 0; g < n; ++g) total += cs[g]->cnt.total;
    const uint32_t P = rc_count_plan(total);
    // histograms: occurrences per slice on every GPU
    std::vector<std::vector<unsigned long long>> hist((size_t)n, std::vector<unsigned long long>(64, 0));
    {
        std::vector<rc_dev_tmp> b_hist((size_t)n);
        for (int g = 0; g < n; ++g) {
            RC_CHECK_HIP(c0, hipSetDevice(cs[g]->device));
            RC_CHECK_HIP(c0, b_hist[(size_t)g].alloc(64 * 8));
            RC_CHECK_HIP(c0, hipMemsetAsync(b_hist[(size_t)g].p, 0, 64 * 8, cs[g]->stream));
            rc_count_scan<0>(cs[g]->cnt.arenas, cs[g]->stream, k, P, 0u, b_hist[(size_t)g].as<unsigned long long>(), nullptr, nullptr);
            RC_CHECK_HIP(c0, hipGetLastError());
            RC_CHECK_HIP(c0, hipMemcpyAsync(hist[(size_t)g].data(), b_hist[(size_t)g].p, 64 * 8, hipMemcpyDeviceToHost, cs[g]->stream));
        }
        for (int g = 0; g < n; ++g) {
            RC_CHECK_HIP(c0, hipSetDevice(cs[g]->device));
            RC_CHECK_HIP(c0, hipStreamSynchronize(cs[g]->stream));
        }
    }
    std::vector<size_t> slice_total(P, 0);
    for (uint32_t p = 0; p < P; ++p)
        for (int g = 0; g < n; ++g) slice_total[p] += (size_t)hist[(size_t)g][p];
    // per owner: the scratch of its largest slice; per GPU: a staging buffer for the keys it emits for someone else
    struct Owner {
        rc_slice_scratch S;
        rc_kept_arrays K;
        rc_dev_tmp spec;
        size_t max_slice = 0;
    };
    std::vector<Owner> own((size_t)n);
    std::vector<rc_dev_tmp> stage((size_t)n), cursor((size_t)n);
    std::vector<size_t> stage_each((size_t)n, 0);
    const uint32_t spec_bin = c0->spec_arm;
    for (int g = 0; g < n; ++g) {
        Owner &O = own[(size_t)g];
        size_t max_emit = 0;
        for (uint32_t p = 0; p < P; ++p) {
            if ((int)(p % (uint32_t)n) == g) O.max_slice = std::max(O.max_slice, slice_total[p]);
            else max_emit = std::max(max_emit, (size_t)hist[(size_t)g][p]);
        }
        if (O.max_slice >= (1ull << 32)) {
            rc_set_error(c0, "count: a pass of %zu k-mer occurrences exceeds 2^32 (lower RC_COUNT_MEM_MB for more passes)", O.max_slice);
            return RC_ERR_ARG;
        }
        RC_CHECK_HIP(c0, hipSetDevice(cs[g]->device));
        RC_CHECK_HIP(c0, cursor[(size_t)g].alloc((size_t)n * 8));  // one cursor and one staging buffer per owner of a round
        stage_each[(size_t)g] = max_emit;
        if (max_emit) RC_CHECK_HIP(c0, stage[(size_t)g].alloc((size_t)n * max_emit * 8));
        if (O.max_slice == 0) continue;
        const int ra = O.S.alloc(c0, O.max_slice, k, cs[g]->stream);
        if (ra) return ra;
        if (spec_bin) {  // (rc_table_count_spectrum on ctxs[0]: every owner sums the spectrum of its slices)
            RC_CHECK_HIP(c0, O.spec.alloc(((size_t)spec_bin + 5) * 8));
            RC_CHECK_HIP(c0, hipMemsetAsync(O.spec.p, 0, ((size_t)spec_bin + 5) * 8, cs[g]->stream));
        }
    }
    auto sync_all = [&]() -> int {
        for (int g = 0; g < n; ++g) {
            RC_CHECK_HIP(c0, hipSetDevice(cs[g]->device));
            RC_CHECK_HIP(c0, hipStreamSynchronize(cs[g]->stream));
        }
        return RC_OK;
    };
    // rounds: in round r GPU o owns slice r n + o
    struct Piece {
        int owner;
        size_t at, n;
    };
    std::vector<Piece> pieces(P, Piece{0, 0, 0});  // where slice p's kept entries lie in its owner's arrays
    for (uint32_t r0 = 0; r0 < P; r0 += (uint32_t)n) {
        // every GPU emits, for every owner of this round, the slice's keys from its own arenas: its own slice straight into its
        // sort buffer, the others' into a staging buffer each -- all GPUs at once, nothing waits for the host
        auto before_of = [&](int g, uint32_t p) {  // a GPU's keys follow those of the GPUs before it
            size_t b = 0;
            for (int h = 0; h < g; ++h) b += (size_t)hist[(size_t)h][p];
            return b;
        };
        for (int g = 0; g < n; ++g) {
            RC_CHECK_HIP(c0, hipSetDevice(cs[g]->device));
            RC_CHECK_HIP(c0, hipMemsetAsync(cursor[(size_t)g].p, 0, (size_t)n * 8, cs[g]->stream));
            for (int o = 0; o < n; ++o) {
                const uint32_t p = r0 + (uint32_t)o;
                if (p >= P) break;
                if (hist[(size_t)g][p] == 0) continue;
                uint64_t *dst_local = g == o ? own[(size_t)o].S.keys + before_of(g, p) : stage[(size_t)g].as<uint64_t>() + (size_t)o * stage_each[(size_t)g];
                rc_count_scan<1>(cs[g]->cnt.arenas, cs[g]->stream, k, P, p, nullptr, dst_local, cursor[(size_t)g].as<unsigned long long>() + o);
                RC_CHECK_HIP(c0, hipGetLastError());
            }
        }
        int rc = sync_all();
        if (rc) return rc;
        // ... and every owner fetches what the others emitted for it (the owners' streams side by side)
        for (int o = 0; o < n; ++o) {
            const uint32_t p = r0 + (uint32_t)o;
            if (p >= P) break;
            RC_CHECK_HIP(c0, hipSetDevice(cs[o]->device));
            for (int g = 0; g < n; ++g) {
                const size_t m = (size_t)hist[(size_t)g][p];
                if (g == o || m == 0) continue;
                rc = rc_copy_across(c0, own[(size_t)o].S.keys + before_of(g, p), cs[o]->device, stage[(size_t)g].as<uint64_t>() + (size_t)o * stage_each[(size_t)g],
                                    cs[g]->device, m * 8, cs[o]->stream, "count: copy between GPUs");
                if (rc) return rc;
            }
        }
        rc = sync_all();
        if (rc) return rc;
        // every owner reduces its slice (the owners' streams run side by side; the host waits for each in turn)
        std::vector<size_t> runs((size_t)n, 0), nsel((size_t)n, 0);
        for (int phase = 0; phase < 3; ++phase)
            for (int o = 0; o < n; ++o) {
                const uint32_t p = r0 + (uint32_t)o;
                if (p >= P || slice_total[p] == 0) continue;
                Owner &O = own[(size_t)o];
                hipStream_t st = cs[o]->stream;
                RC_CHECK_HIP(c0, hipSetDevice(cs[o]->device));
                if (phase == 0) {
                    rc = rc_slice_reduce(c0, O.S, slice_total[p], st, &runs[(size_t)o], nullptr);
                    if (rc) return rc;
                } else if (phase == 1) {
                    RC_CHECK_HIP(c0, hipStreamSynchronize(st));
                    if (runs[(size_t)o] == 0) continue;
                    rc = rc_slice_select(c0, O.S, runs[(size_t)o], min_count, spec_bin, O.spec.as<unsigned long long>(), st, &nsel[(size_t)o]);
                    if (rc) return rc;
                } else {
                    RC_CHECK_HIP(c0, hipStreamSynchronize(st));
                    const size_t ns = runs[(size_t)o] ? nsel[(size_t)o] : 0;
                    pieces[p] = Piece{o, O.K.n, ns};
                    if (ns == 0) continue;
                    // (the arrays' size: what this owner has kept of what it has seen, applied to what it has still to see, + 50 %)
                    size_t seen = 0, todo = 0;
                    for (uint32_t q = (uint32_t)o; q < P; q += (uint32_t)n) (q <= p ? seen : todo) += slice_total[q];
                    const size_t want = (size_t)((double)(O.K.n + ns) * (1.0 + 1.5 * (double)todo / (double)(seen ? seen : 1))) + ((size_t)1 << 16);
                    rc = rc_kept_append(c0, O.K, O.S, runs[(size_t)o], ns, want, st, nullptr);
                    if (rc) return rc;
                }
            }
        rc = sync_all();
        if (rc) return rc;
    }
    if (spec_bin) {  // every owner's few KB back to the host, summed (the slices are disjoint in key space)
        std::vector<uint64_t> sum((size_t)spec_bin + 5, 0), f((size_t)spec_bin + 5);
        for (int g = 0; g < n; ++g) {
            if (!own[(size_t)g].spec.p) continue;
            RC_CHECK_HIP(c0, hipSetDevice(cs[g]->device));
            RC_CHECK_HIP(c0, hipMemcpyAsync(f.data(), own[(size_t)g].spec.p, f.size() * 8, hipMemcpyDeviceToHost, cs[g]->stream));
            RC_CHECK_HIP(c0, hipStreamSynchronize(cs[g]->stream));
            const size_t mc = (size_t)spec_bin + 4;  // (max_count: a maximum, the rest sums)
            for (size_t i = 0; i < mc; ++i) sum[i] += f[i];
            sum[mc] = std::max(sum[mc], f[mc]);
            own[(size_t)g].spec.reset();
        }
        c0->spec_counted = std::move(sum);
    }
    // the kept entries, slice after slice, on cs[0]
    rc_kept_arrays all;
    for (uint32_t p = 0; p < P; ++p) all.n += pieces[p].n;
    RC_CHECK_HIP(c0, hipSetDevice(c0->device));
    RC_CHECK_HIP(c0, all.k.alloc((all.n + 1) * 8));
    RC_CHECK_HIP(c0, all.c.alloc((all.n + 1) * 4));
    {
        size_t at = 0;
        for (uint32_t p = 0; p < P; ++p) {
            const Piece &pc = pieces[p];
            if (pc.n == 0) continue;
            const rc_kept_arrays &K = own[(size_t)pc.owner].K;
            int rc = rc_copy_across(c0, all.k.as<uint64_t>() + at, c0->device, K.k.as<uint64_t>() + pc.at, cs[pc.owner]->device, pc.n * 8, c0->stream, "count: copy between GPUs");
            if (!rc) rc = rc_copy_across(c0, all.c.as<int32_t>() + at, c0->device, K.c.as<int32_t>() + pc.at, cs[pc.owner]->device, pc.n * 4, c0->stream, "count: copy between GPUs");
            if (rc) return rc;
            at += pc.n;
        }
        RC_CHECK_HIP(c0, hipStreamSynchronize(c0->stream));
    }
    for (int g = 0; g < n; ++g) {  // scratch back to its device; the reads stay where they are for rc_submit_resident, if asked
        RC_CHECK_HIP(c0, hipSetDevice(cs[g]->device));
        own[(size_t)g].S.pool.reset();
        own[(size_t)g].K.k.reset();
        own[(size_t)g].K.c.reset();
        stage[(size_t)g].reset();
        cursor[(size_t)g].reset();
        rc_count_end(cs[g], c0->cnt_keep);
    }
    RC_CHECK_HIP(c0, hipSetDevice(c0->device));
    const int rc = rc_count_build(c0, all, n_kmers);
    if (rc != RC_OK)
        for (int g = 0; g < n; ++g) {
            (void)hipSetDevice(cs[g]->device);
            cs[g]->kept.release();
        }
    (void)hipSetDevice(c0->device);
    return rc;
}
