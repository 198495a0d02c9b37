// rc_table.hip -- the k-mer count table in HBM (Store.h:17-88 re-designed for the MI355X memory
// system) and the kernels that touch only the table: build (K0), lookup, the per-batch probe
// kernel (K1: reads -> counts[], ErrorCorrection.cpp:716-723), the k-mer count spectrum and
// census, and the last-base-variant pass of the ERROR_RATE estimation (main.cpp:329-345).  The
// k-mer counter that feeds the build (stages 0-2 of run_rcorrector.pl:262-281) is rc_count.hip.
//
// Layout: open addressing over 64-byte buckets (one HBM/L2 sector per probe): 5 slots of
// {key_lo, key_hi, count} + one meta dword.  A key lives in its home bucket hash(key) & mask or,
// if that is full, in the following buckets (no wrap-around: the array carries slack buckets).
// meta bit0 of bucket b says "some key with home <= b was placed after b", so a miss stops at
// the first bucket without that bit -- >96 % of all probes, hit or miss, touch exactly one
// bucket at the load factors used (<= 0.5).
//
// The build is a sort, not a race: entries are stably radix-sorted by home bucket (input order
// reversed so that of two equal keys the LATER one is met first by a probe, which is the
// "later Put overwrites" rule of Store.h:55), slot numbers come from one prefix-max scan
// p_j = max(5*home_j, p_{j-1}+1), and a scatter writes the buckets.  The layout is therefore a
// pure function of the input, independent of thread timing.
#include <cstring>
#include <vector>

#include <algorithm>
#include <vector>
#include <rocprim/rocprim.hpp>

#include <chrono>
#include "rc_internal.h"
#include "rc_device.h"

// ---- K0: build -----------------------------------------------------------------------------
__global__ void k_home_and_index(const uint64_t *__restrict__ canon, uint32_t *__restrict__ home,
                                 uint32_t *__restrict__ idx, size_t n, uint32_t nb_home, int layout, int k, int ext)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    size_t i = n - 1 - j;  // reversed input order (see header)
    uint32_t h, rem, xrem;
    if (layout)
        rc_packed_addr(canon[i], k, nb_home, ext, &h, &rem, &xrem);
    else
        h = rc_home(canon[i], nb_home);
    home[j] = h;
    idx[j] = (uint32_t)i;
}

__global__ void k_slot_seed(const uint32_t *__restrict__ home_sorted, long long *__restrict__ q, size_t n, int slots)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    q[j] = (long long)slots * home_sorted[j] - (long long)j;
}

// what rules the PACKED layout out for a given input: a key pushed more than 14 buckets past its home
// (flags[0] |= 2), or more counts that do not fit the count field than the table's prefix holds
// (flags[1] = how many there are: rc_common.h, RC_PACKED_OVF_MAX).
__global__ void k_packed_feasible(const uint32_t *__restrict__ home_sorted, const long long *__restrict__ qmax,
                                  const int32_t *__restrict__ counts, size_t n, int ext, unsigned *__restrict__ flags)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long p = qmax[j] + (long long)j;
    if ((uint32_t)counts[j] >= (RC_PACKED_COUNT_MASK >> ext)) atomicAdd(flags + 1, 1u);  // (counts are indexed by input, any order does)
    if ((uint32_t)(p / RC_PACKED_SLOTS) - home_sorted[j] > RC_PACKED_MAX_DISP) atomicOr(flags, 2u);
}

// the entries whose count does not fit: {code, count, input index} in any order (the host sorts the few)
__global__ void k_collect_overflow(const uint64_t *__restrict__ canon, const int32_t *__restrict__ counts, size_t n, uint32_t cmask,
                                   unsigned *__restrict__ n_out, uint4 *__restrict__ out, uint32_t *__restrict__ out_idx)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n || (uint32_t)counts[i] < cmask) return;
    const unsigned o = atomicAdd(n_out, 1u);
    if (o >= RC_PACKED_OVF_MAX) return;
    out[o] = make_uint4((uint32_t)canon[i], (uint32_t)(canon[i] >> 32), (uint32_t)counts[i], 0u);
    out_idx[o] = (uint32_t)i;
}

__global__ void k_scatter(const uint32_t *__restrict__ home_sorted, const uint32_t *__restrict__ idx_sorted,
                          const long long *__restrict__ qmax, const uint64_t *__restrict__ canon,
                          const int32_t *__restrict__ counts, uint32_t *__restrict__ buckets, size_t n, uint32_t nb_home, int layout, int k, int ext)
{
    size_t j = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= n) return;
    const long long p = qmax[j] + (long long)j;
    const int S = rc_layout_slots(layout);
    const uint32_t b = (uint32_t)(p / S), s = (uint32_t)(p % S);
    const uint32_t i = idx_sorted[j];
    const uint64_t key = canon[i];
    if (layout) {
        uint32_t h, rem, xrem;
        rc_packed_addr(key, k, nb_home, ext, &h, &rem, &xrem);
        uint32_t *w = buckets + (size_t)b * RC_BUCKET_DWORDS + s * 2;
        w[0] = rem;
        // the last slot's bit 31 is the bucket's continue flag, set (atomically: another thread may own
        // that slot) by whoever lands in slot 0 of the next bucket with an earlier home
        atomicAnd(w + 1, 0x80000000u);  // (the slot starts as RC_PACKED_EMPTY_WORD; the flag bit may already be set)
        const uint32_t cmask = RC_PACKED_COUNT_MASK >> ext, cnt = (uint32_t)counts[i] < cmask ? (uint32_t)counts[i] : cmask;  // all ones: see the prefix
        atomicOr(w + 1, cnt | (xrem << (27 - ext)) | ((b - h) << 27));
        if (s == 0 && h < b) atomicOr(buckets + (size_t)(b - 1) * RC_BUCKET_DWORDS + (RC_BUCKET_DWORDS - 1), 0x80000000u);
    } else {
        uint32_t *w = buckets + (size_t)b * RC_BUCKET_DWORDS + s * 3;
        w[0] = (uint32_t)key;
        w[1] = (uint32_t)(key >> 32);
        w[2] = (uint32_t)counts[i];
        if (s == 0 && home_sorted[j] < b) buckets[(size_t)(b - 1) * RC_BUCKET_DWORDS + (RC_BUCKET_DWORDS - 1)] = 1u;
    }
}

// the absence filter of a PACKED table (rc_common.h: rc_table_view::filter): every entry sets its three bits -- kind 1: under
// both of its orientations
__global__ void k_filter_set(const uint64_t *__restrict__ canon, size_t n, uint32_t nb_home, int k, int ext, uint32_t *__restrict__ filter, uint32_t words,
                             int kind)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (kind) {
        const uint64_t x = canon[i], rv = rc_revcomp(x, k);
        uint32_t w, m;
        rc_filter_core_addr(x, words, &w, &m);
        atomicOr(filter + w, m);
        if (rv != x) {
            rc_filter_core_addr(rv, words, &w, &m);
            atomicOr(filter + w, m);
        }
        return;
    }
    uint32_t h, rem, xrem, top;
    rc_packed_addr(canon[i], k, nb_home, ext, &h, &rem, &xrem, &top);
    atomicOr(filter + rc_mulhi32(top, words), rc_filter_mask(rem));
}

// one attempt at one layout; *ok = false (PACKED only) if a count or a displacement does not fit
static int build_attempt(rc_ctx *ctx, const uint64_t *d_canon, const int32_t *d_counts, size_t n, int layout, int ext, uint32_t nb_home, bool *ok)
{
    *ok = true;
    const int S = rc_layout_slots(layout);
    int bits = 0;
    while ((1ull << bits) < (uint64_t)nb_home) ++bits;
    long long p_last = -1;
    unsigned n_overflow = 0;  // PACKED: counts that go to the table's prefix
    rc_dev_tmp b_home, b_home_s, b_idx, b_idx_s, b_q, b_qm, b_tmp, b_flags;
    const unsigned B = 256;
    const unsigned G = (unsigned)((n + B - 1) / B);
    if (n > 0) {
        size_t tmp_sort = 0, tmp_scan = 0;
        RC_CHECK_HIP(ctx, b_home.alloc(n * 4));
        RC_CHECK_HIP(ctx, b_home_s.alloc(n * 4));
        RC_CHECK_HIP(ctx, b_idx.alloc(n * 4));
        RC_CHECK_HIP(ctx, b_idx_s.alloc(n * 4));
        RC_CHECK_HIP(ctx, b_q.alloc(n * 8));
        RC_CHECK_HIP(ctx, b_qm.alloc(n * 8));
        RC_CHECK_HIP(ctx, b_flags.alloc(8));
        uint32_t *home = b_home.as<uint32_t>(), *home_s = b_home_s.as<uint32_t>();
        uint32_t *idx = b_idx.as<uint32_t>(), *idx_s = b_idx_s.as<uint32_t>();
        long long *q = b_q.as<long long>(), *qm = b_qm.as<long long>();
        hipLaunchKernelGGL(k_home_and_index, dim3(G), dim3(B), 0, ctx->stream, d_canon, home, idx, n, nb_home, layout, ctx->k, ext);
        RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, tmp_sort, home, home_s, idx, idx_s, n, 0, bits > 0 ? bits : 1, ctx->stream));
        RC_CHECK_HIP(ctx, rocprim::inclusive_scan(nullptr, tmp_scan, q, qm, n, rocprim::maximum<long long>(), ctx->stream));
        RC_CHECK_HIP(ctx, b_tmp.alloc(tmp_sort > tmp_scan ? tmp_sort : tmp_scan));
        RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(b_tmp.p, tmp_sort, home, home_s, idx, idx_s, n, 0, bits > 0 ? bits : 1, ctx->stream));
        hipLaunchKernelGGL(k_slot_seed, dim3(G), dim3(B), 0, ctx->stream, home_s, q, n, S);
        RC_CHECK_HIP(ctx, rocprim::inclusive_scan(b_tmp.p, tmp_scan, q, qm, n, rocprim::maximum<long long>(), ctx->stream));
        long long q_last = 0;
        unsigned flags[2] = {0, 0};
        if (layout) {
            RC_CHECK_HIP(ctx, hipMemsetAsync(b_flags.p, 0, 8, ctx->stream));
            hipLaunchKernelGGL(k_packed_feasible, dim3(G), dim3(B), 0, ctx->stream, home_s, qm, d_counts, n, ext, b_flags.as<unsigned>());
            RC_CHECK_HIP(ctx, hipMemcpyAsync(flags, b_flags.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        RC_CHECK_HIP(ctx, hipMemcpyAsync(&q_last, qm + (n - 1), 8, hipMemcpyDeviceToHost, ctx->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (flags[0] || flags[1] > RC_PACKED_OVF_MAX) {
            *ok = false;
            return RC_OK;
        }
        n_overflow = flags[1];
        p_last = q_last + (long long)(n - 1);
    }
    uint64_t need = (uint64_t)(p_last / S) + 2;  // +1 empty bucket after the last used
    uint64_t nb_alloc = need > (uint64_t)nb_home + 1 ? need : (uint64_t)nb_home + 1;
    if (nb_alloc >= (1ull << 32)) {
        rc_set_error(ctx, "table build: bucket count overflow");
        return RC_ERR_ARG;
    }
    ctx->nb_home = nb_home;
    ctx->layout = layout;
    ctx->ext = layout ? ext : 0;
    ctx->nb_alloc = (uint32_t)nb_alloc;
    ctx->table_bytes = (size_t)nb_alloc * RC_BUCKET_BYTES;
    // A bucket array beyond the reach of the TLB (2.7-3.2 GB on the boxes seen) makes every probe a page walk, and most
    // probes of the search -- 61 % at 0.5 % errors, 72 % at 5 % -- are of k-mers that are not in the table at all: a
    // filter of 10 bits per entry behind the buckets (a tenth of their size, inside the TLB's reach up to ~2.5 G
    // entries) answers those without touching the buckets.  PACKED tables beyond 2.5 GiB only: below, a bucket read
    // costs what a filter word costs.  RC_TABLE_FILTER=force / off for tests and A/B runs.
    // RC_TABLE_FILTER_KIND=plain|core: how a k-mer finds its word (rc_common.h: rc_table_view::filter_kind); RC_TABLE_FILTER=search:
    // the filter of a mid-size table (the search's lookups only) on a table of any size (tests).
    ctx->filter_words = 0;
    {
        const char *e = getenv("RC_TABLE_FILTER"), *kd = getenv("RC_TABLE_FILTER_KIND");
        const bool force = e && !strcmp(e, "force"), off = e && !strcmp(e, "off"), search = e && !strcmp(e, "search");
        ctx->filter_kind = kd ? (strcmp(kd, "plain") != 0 ? 1 : 0) : RC_FILTER_KIND_DEFAULT;
        // beyond 2.5 GiB every lookup asks the filter.  RC_TABLE_FILTER=search (dev): a core filter that only the search's
        // lookups ask, on a table of any size -- measured on the tables inside the TLB's reach and not taken: k_correct is
        // bound by instruction issue there, and the filter's hash costs it more than the bucket reads it saves (config 2:
        // 20.1 / 20.3 ms against 19.6 / 19.5; config 3: 53.1 / 51.8 against 51.3 / 49.4; profiles/r5_search_filter_ab.txt)
        const bool big = ctx->table_bytes > ((size_t)5 << 29);
        const bool mid = ctx->filter_kind == 1 && search;
        ctx->filter_all = (force || big) ? 1 : 0;
        if (layout && n > 0 && !off && (force || big || mid)) {
            uint64_t bits = ctx->filter_kind ? 16 : 10;  // per entry
            if (const char *fb = getenv("RC_TABLE_FILTER_BITS")) bits = (uint64_t)atoi(fb) >= 4 ? (uint64_t)atoi(fb) : bits;  // dev
            uint64_t w = ((uint64_t)n * bits + 31) / 32 + 64;
            if (w < (1ull << 32)) ctx->filter_words = (uint32_t)w;
        }
    }
    const size_t filter_bytes = (size_t)ctx->filter_words * 4;
    {   // the bucket array, RC_TABLE_PREFIX_BYTES (zero unless counts overflow, below) in front of it, the filter behind it
        char *base = nullptr;
        RC_CHECK_HIP(ctx, hipMalloc((void **)&base, ctx->table_bytes + RC_TABLE_PREFIX_BYTES + filter_bytes));  // (hipDeviceMallocContiguous: no effect on the TLB cliff, measured)
        ctx->d_buckets = reinterpret_cast<uint32_t *>(base + RC_TABLE_PREFIX_BYTES);
        RC_CHECK_HIP(ctx, hipMemsetAsync(base, 0, RC_TABLE_PREFIX_BYTES, ctx->stream));
        if (filter_bytes) RC_CHECK_HIP(ctx, hipMemsetAsync(base + RC_TABLE_PREFIX_BYTES + ctx->table_bytes, 0, filter_bytes, ctx->stream));
    }
    if (layout && n_overflow) {
        rc_dev_tmp b_o, b_oi, b_on;
        RC_CHECK_HIP(ctx, b_o.alloc(RC_PACKED_OVF_MAX * sizeof(uint4)));
        RC_CHECK_HIP(ctx, b_oi.alloc(RC_PACKED_OVF_MAX * 4));
        RC_CHECK_HIP(ctx, b_on.alloc(4));
        RC_CHECK_HIP(ctx, hipMemsetAsync(b_on.p, 0, 4, ctx->stream));
        hipLaunchKernelGGL(k_collect_overflow, dim3(G), dim3(B), 0, ctx->stream, d_canon, d_counts, n, RC_PACKED_COUNT_MASK >> ext, b_on.as<unsigned>(),
                           b_o.as<uint4>(), b_oi.as<uint32_t>());
        std::vector<uint4> e(n_overflow);
        std::vector<uint32_t> ei(n_overflow);
        RC_CHECK_HIP(ctx, hipMemcpyAsync(e.data(), b_o.p, n_overflow * sizeof(uint4), hipMemcpyDeviceToHost, ctx->stream));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(ei.data(), b_oi.p, n_overflow * 4, hipMemcpyDeviceToHost, ctx->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        // ascending by code; of two Puts of one code the later one is the table's entry (Store.h:55)
        std::vector<uint32_t> o(n_overflow);
        for (uint32_t i = 0; i < n_overflow; ++i) o[i] = i;
        auto code = [&](uint32_t i) { return ((uint64_t)e[i].y << 32) | e[i].x; };
        std::sort(o.begin(), o.end(), [&](uint32_t a, uint32_t b) { return code(a) != code(b) ? code(a) < code(b) : ei[a] < ei[b]; });
        std::vector<uint4> sorted;
        for (uint32_t j = 0; j < n_overflow; ++j)
            if (j + 1 == n_overflow || code(o[j + 1]) != code(o[j])) sorted.push_back(e[o[j]]);
        const uint32_t ns = (uint32_t)sorted.size();
        char *base = reinterpret_cast<char *>(ctx->d_buckets) - RC_TABLE_PREFIX_BYTES;
        RC_CHECK_HIP(ctx, hipMemcpyAsync(base, sorted.data(), ns * sizeof(uint4), hipMemcpyHostToDevice, ctx->stream));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(reinterpret_cast<char *>(ctx->d_buckets) - 64, &ns, 4, hipMemcpyHostToDevice, ctx->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));  // (the vectors go out of scope)
    }
    if (layout)
        RC_CHECK_HIP(ctx, hipMemsetD32Async((hipDeviceptr_t)ctx->d_buckets, (int)RC_PACKED_EMPTY_WORD, ctx->table_bytes / 4, ctx->stream));
    else
        RC_CHECK_HIP(ctx, hipMemsetAsync(ctx->d_buckets, 0, ctx->table_bytes, ctx->stream));
    if (n > 0) {
        hipLaunchKernelGGL(k_scatter, dim3(G), dim3(B), 0, ctx->stream, b_home_s.as<uint32_t>(), b_idx_s.as<uint32_t>(),
                           b_qm.as<long long>(), d_canon, d_counts, ctx->d_buckets, n, nb_home, layout, ctx->k, ext);
        if (ctx->filter_words)
            hipLaunchKernelGGL(k_filter_set, dim3(G), dim3(B), 0, ctx->stream, d_canon, n, nb_home, ctx->k, ext,
                               ctx->d_buckets + ctx->table_bytes / 4, ctx->filter_words, ctx->filter_kind);
        RC_CHECK_HIP(ctx, hipGetLastError());
    }
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->n_entries = n;
    return RC_OK;
}

int rc_build_table_from_device_pairs(rc_ctx *ctx, const uint64_t *d_canon, const int32_t *d_counts, size_t n)
{
    if (n >= (1ull << 31)) {
        rc_set_error(ctx, "table build: %zu entries exceed the 2^31 limit", n);
        return RC_ERR_ARG;
    }
    rc_table_release(ctx);
    // home buckets: n / (slots * load).  Random 64-byte gathers on MI355X are request-rate bound
    // (~55 G/s, tools/microbench_gather.hip) and fall off a cliff once the table outgrows the TLB
    // reach (~2 GiB), so a dense table wins: fewer bytes => more MALL/L2 hits per probe.
    auto buckets_for = [&](int slots, double load, double dflt) -> uint64_t {
        if (!(load > 0.05 && load <= 0.95)) load = dflt;
        uint64_t want = (uint64_t)((double)n / (slots * load)) + 1;
        return want < 64 ? 64 : want;
    };
    // PACKED needs nb_home * 2^ext >= 2^(2k-32) for (home, rem, xrem) to identify a code: ext = the
    // smallest such number of extra remainder bits (0 for k <= 28 at ordinary table sizes); it is
    // used when at most RC_PACKED_MAX_EXT are needed and the placement allows (k_packed_feasible), WIDE otherwise
    // load by size: the emptier the table, the fewer probes run on into a second bucket (configs 1-3 at
    // 0.4 / 0.45 / 0.5: 282 / 281 / 275, 201 / 201 / 197 and 212 / 210 / 206 M reads/s; 0.6 / 0.7 / 0.8:
    // config 2 at 187 / 174 / 145) -- until the table leaves the reach of the TLB, 2.7-3.2 GB depending on
    // the box: 201 M entries at 0.5 / 0.6 / 0.65 / 0.7 = 3.2 / 2.7 / 2.5 / 2.3 GB: k_correct 1537 / 1189 / 1227 /
    // 1280 ms.  So: 0.4 up to 2 GiB, 0.5 up to 2.5 GiB, 0.6 beyond.
    double packed_load = ctx->table_load_packed;
    if (!ctx->table_load_set) {
        const double gib = (double)n * 8.0 / 1073741824.0;  // slot bytes of the entries
        packed_load = gib / 0.40 <= 2.0 ? 0.40 : (gib / 0.50 <= 2.5 ? 0.50 : 0.60);
    }
    const uint64_t packed = buckets_for(RC_PACKED_SLOTS, packed_load, 0.50);
    const int kb = 2 * ctx->k;
    int ext = 0;
    while (kb > 32 && kb - 32 - ext > 0 && (packed << ext) < (1ull << (kb - 32))) ++ext;
    if (ctx->layout_pref != 0 && ext <= RC_PACKED_MAX_EXT && packed < (1ull << 32) - 8) {
        bool ok = false;
        int rc = build_attempt(ctx, d_canon, d_counts, n, 1, ext, (uint32_t)packed, &ok);
        if (rc) return rc;
        if (ok) return RC_OK;  // else: too many counts beyond the count field or a chain longer than 15 buckets -- WIDE takes anything
    }
    // WIDE: past the reach of the TLB (a table of 4.9 GB: two L1-TLB misses in three requests) a
    // denser table is worth its longer probe chains -- 201 M entries, 25 M x 150 bp reads at 5 % errors:
    // k_correct 2412 / 2257 / 2024 / 1841 / 1874 / 2551 ms at load 0.5 / 0.6 / 0.65 / 0.7 / 0.75 / 0.8
    double wide_load = ctx->table_load;
    if (!ctx->table_load_set && (double)n / (RC_WIDE_SLOTS * 0.50) * RC_BUCKET_BYTES > 3.0 * 1073741824.0) wide_load = 0.70;
    const uint64_t wide = buckets_for(RC_WIDE_SLOTS, wide_load, 0.50);
    if (wide >= (1ull << 32) - 8) {
        rc_set_error(ctx, "table build: bucket count overflow");
        return RC_ERR_ARG;
    }
    bool ok = false;
    return build_attempt(ctx, d_canon, d_counts, n, 0, 0, (uint32_t)wide, &ok);
}

// forward (or canonical) reference codes -> canonical, in place
__global__ void k_canonicalize(uint64_t *codes, size_t n, int k)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) codes[i] = rc_canonical(codes[i], k);
}

int rc_launch_canonicalize(rc_ctx *ctx, uint64_t *d_codes, size_t n)
{
    if (n == 0) return RC_OK;
    hipLaunchKernelGGL(k_canonicalize, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_codes, n, ctx->k);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// Store::GetCount for an array of VALID forward/canonical codes (Store.h:59-66)
__global__ void k_lookup(rc_table_view T, const uint64_t *__restrict__ codes, size_t n, int k, int32_t *__restrict__ out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = rc_table_lookup(T, rc_canonical(codes[i], k));
}

int rc_launch_lookup(rc_ctx *ctx, const uint64_t *d_codes, size_t n, int32_t *d_out)
{
    if (n == 0) return RC_OK;
    hipLaunchKernelGGL(k_lookup, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rc_view(ctx), d_codes, n, ctx->k, d_out);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// main.cpp:329-345: for every dump entry, the counts of its four last-base variants in A,C,G,T
// order, reduced to (max, secondMax) with the reference's tie rule.  out[2*i] = max, [2*i+1] = second.
__global__ void k_last_base_variants(rc_table_view T, const uint64_t *__restrict__ codes, size_t n, int k,
                                     int32_t *__restrict__ out)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t base = codes[i] & ~3ull;
    int mx = 0, second = 0;
    for (int c = 0; c < 4; ++c) {
        int cnt = rc_table_lookup_o(T, rc_canonical(base | (uint64_t)c, k), base | (uint64_t)c);  // (the four variants share a filter word)
        if (cnt > mx) {
            second = mx;
            mx = cnt;
        } else if (cnt > second)
            second = cnt;
    }
    out[2 * i] = mx;
    out[2 * i + 1] = second;
}

int rc_launch_last_base_variants(rc_ctx *ctx, const uint64_t *d_codes, size_t n, int32_t *d_max2)
{
    if (n == 0) return RC_OK;
    hipLaunchKernelGGL(k_last_base_variants, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rc_view(ctx), d_codes, n, ctx->k, d_max2);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// The entries the ERROR_RATE scan keeps (main.cpp:329-347: max >= 1000), picked on the device: of n dump entries only these
// few matter, and only the first 100 000 of them in dump order.  out_key = the entry's place in that order (its index in
// the file, or rc_dump_order_key of its code for a table that was counted here), out_val = max << 32 | second.  n_out
// counts every kept entry, the arrays hold the first `cap` in no particular order (the caller sorts by key).
__global__ __launch_bounds__(256) void k_error_rate_candidates(rc_table_view T, const uint64_t *__restrict__ codes, size_t n, int k, int by_hash,
                                                               uint64_t *__restrict__ out_key, uint64_t *__restrict__ out_val,
                                                               unsigned long long *__restrict__ n_out, size_t cap)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    int mx = 0, second = 0;
    uint64_t code = 0;
    if (i < n) {
        code = codes[i];
        const uint64_t base = code & ~3ull;
        for (int c = 0; c < 4; ++c) {
            int cnt = rc_table_lookup_o(T, rc_canonical(base | (uint64_t)c, k), base | (uint64_t)c);  // (the four variants share a filter word)
            if (cnt > mx) {
                second = mx;
                mx = cnt;
            } else if (cnt > second)
                second = cnt;
        }
    }
    const bool keep = i < n && mx >= 1000;
    const unsigned long long m = __ballot(keep);
    if (!m) return;
    const int lane = threadIdx.x & 63, leader = __ffsll((long long)m) - 1;
    unsigned long long base_at = 0;
    if (lane == leader) base_at = atomicAdd(n_out, (unsigned long long)__popcll(m));
    base_at = __shfl(base_at, leader, 64);
    if (keep) {
        const unsigned long long at = base_at + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (at < cap) {
            out_key[at] = by_hash ? rc_dump_order_key(code) : (uint64_t)i;
            out_val[at] = ((uint64_t)(uint32_t)mx << 32) | (uint32_t)second;
        }
    }
}

// the (max, second) pairs of the first `want` kept entries in dump order
int rc_error_rate_candidates(rc_ctx *ctx, const uint64_t *d_codes, size_t n, bool by_hash, size_t want, std::vector<uint64_t> *vals)
{
    vals->clear();
    if (n == 0) return RC_OK;
    rc_dev_tmp b_key, b_val, b_key_s, b_val_s, b_n, b_tmp;
    RC_CHECK_HIP(ctx, b_n.alloc(8));
    size_t cap = std::min<size_t>(n, (size_t)4 << 20);
    unsigned long long found = 0;
    for (int attempt = 0; attempt < 2; ++attempt) {
        RC_CHECK_HIP(ctx, b_key.alloc(cap * 8));
        RC_CHECK_HIP(ctx, b_val.alloc(cap * 8));
        RC_CHECK_HIP(ctx, hipMemsetAsync(b_n.p, 0, 8, ctx->stream));
        hipLaunchKernelGGL(k_error_rate_candidates, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, rc_view(ctx), d_codes, n, ctx->k, by_hash ? 1 : 0,
                           b_key.as<uint64_t>(), b_val.as<uint64_t>(), b_n.as<unsigned long long>(), cap);
        RC_CHECK_HIP(ctx, hipGetLastError());
        RC_CHECK_HIP(ctx, hipMemcpyAsync(&found, b_n.p, 8, hipMemcpyDeviceToHost, ctx->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (found <= cap) break;
        cap = (size_t)found;  // (a data set with millions of k-mers beyond 1000: once more with room for all of them)
    }
    const size_t m = (size_t)found;
    if (m == 0) return RC_OK;
    RC_CHECK_HIP(ctx, b_key_s.alloc(m * 8));
    RC_CHECK_HIP(ctx, b_val_s.alloc(m * 8));
    size_t t1 = 0;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t1, b_key.as<uint64_t>(), b_key_s.as<uint64_t>(), b_val.as<uint64_t>(), b_val_s.as<uint64_t>(), m, 0, 64, ctx->stream));
    RC_CHECK_HIP(ctx, b_tmp.alloc(t1));
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(b_tmp.p, t1, b_key.as<uint64_t>(), b_key_s.as<uint64_t>(), b_val.as<uint64_t>(), b_val_s.as<uint64_t>(), m, 0, 64, ctx->stream));
    vals->resize(std::min(m, want));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(vals->data(), b_val_s.p, vals->size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

// the table's canonical codes in HBM, unspecified order: *d_codes is allocated here (hipFree it), *n = their number
int rc_table_codes_device(rc_ctx *ctx, uint64_t **d_codes, size_t *n)
{
    *d_codes = nullptr;
    *n = 0;
    const size_t cap = (size_t)ctx->n_entries;
    if (cap == 0) return RC_OK;
    rc_dev_tmp b_counts, b_n;
    uint64_t *codes = nullptr;
    RC_CHECK_HIP(ctx, hipMalloc((void **)&codes, cap * 8));
    unsigned long long n64 = 0;
    hipError_t e = b_counts.alloc(cap * 4);
    if (e == hipSuccess) e = b_n.alloc(8);
    if (e == hipSuccess) e = hipMemsetAsync(b_n.p, 0, 8, ctx->stream);
    int rc = RC_OK;
    if (e == hipSuccess) rc = rc_launch_export(ctx, codes, b_counts.as<int32_t>(), b_n.as<unsigned long long>(), cap);
    if (e == hipSuccess && rc == RC_OK) e = hipMemcpyAsync(&n64, b_n.p, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess && rc == RC_OK) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || rc != RC_OK || n64 > cap) {
        (void)hipFree(codes);
        if (e != hipSuccess) rc_set_error(ctx, "table export: %s", hipGetErrorString(e));
        else if (rc == RC_OK) rc_set_error(ctx, "table export: %llu entries found, at most %zu expected", n64, cap);
        return e != hipSuccess ? RC_ERR_HIP : (rc != RC_OK ? rc : RC_ERR_STATE);
    }
    *d_codes = codes;
    *n = (size_t)n64;
    return RC_OK;
}

// every stored (canonical code, count) pair, in unspecified order (jf_dump writer / test support)
__global__ void k_export(rc_table_view T, size_t nslots, uint64_t *__restrict__ codes,
                         int32_t *__restrict__ counts, unsigned long long *__restrict__ n_out, size_t cap)
{
    size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nslots) return;
    const int S = rc_layout_slots(T.layout);
    uint64_t key;
    int32_t cnt;
    if (!rc_table_slot_entry(T, s / S, (int)(s % S), &key, &cnt)) return;
    unsigned long long at = atomicAdd(n_out, 1ull);
    if (at < cap) {
        codes[at] = key;
        counts[at] = cnt;
    }
}

// order-independent 64-bit digest of the table's CONTENT (what Store::GetCount can return): the sum
// over live entries of mix(code, count) -- two tables with the same digest answer every probe alike
// whatever their bucket layout (slot format, load factor, build order)
__global__ void k_digest(rc_table_view T, size_t nslots, unsigned long long *__restrict__ out)
{
    size_t s = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long v = 0;
    if (s < nslots) {
        const int S = rc_layout_slots(T.layout);
        uint64_t key;
        int32_t cnt;
        if (rc_table_slot_entry(T, s / S, (int)(s % S), &key, &cnt))
            v = rc_dump_order_key(key ^ rc_dump_order_key((uint64_t)(uint32_t)cnt + 0x9E3779B97F4A7C15ull));
    }
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if ((threadIdx.x & 63) == 0 && v) atomicAdd(out, v);
}

int rc_launch_digest(rc_ctx *ctx, unsigned long long *d_out)
{
    const size_t nslots = (size_t)ctx->nb_alloc * rc_layout_slots(ctx->layout);
    hipLaunchKernelGGL(k_digest, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, ctx->stream, rc_view(ctx), nslots, d_out);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

int rc_launch_export(rc_ctx *ctx, uint64_t *d_codes, int32_t *d_counts, unsigned long long *d_n, size_t cap)
{
    const size_t nslots = (size_t)ctx->nb_alloc * rc_layout_slots(ctx->layout);
    hipLaunchKernelGGL(k_export, dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, ctx->stream, rc_view(ctx), nslots, d_codes, d_counts, d_n, cap);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// ---- k-mer count spectrum (include/rcorrector_amd.h: rc_table_spectrum; accumulate routine in rc_device.h) --------------------
static uint32_t rc_spec_lds_bins(uint32_t max_bin) { return max_bin < RC_SPEC_LDS_BINS ? max_bin + 1 : RC_SPEC_LDS_BINS; }
static size_t rc_spec_lds_bytes(uint32_t lds_bins) { return lds_bins > RC_SPEC_SMALL ? (size_t)(lds_bins - RC_SPEC_SMALL) * 4 : 0; }
#define RC_SPEC_UNROLL 4       // buckets per lane in flight (two 16-byte loads each)
#define RC_SPEC_MAX_BLOCKS 2048

// a PACKED entry stored `disp` buckets behind its home: live iff no slot of the buckets from its home on holds the same key
// (same remainder bits, the displacement of that bucket) -- the first-match rule of rc_table_slot_entry, read from the
// buckets in front of this one (this one's earlier slots were looked at in registers)
__device__ __noinline__ bool rc_spec_packed_first(const rc_table_view &T, size_t b, uint32_t lo, uint32_t hi, uint32_t cmask, uint32_t mhi)
{
    const uint32_t d = (hi >> 27) & 15u;
    const uint32_t key_hi = hi & mhi & ~(15u << 27);
    for (uint32_t j = d; j >= 1; --j) {
        const uint32_t *q = T.buckets + (b - j) * RC_BUCKET_DWORDS;
        const uint32_t want = key_hi | ((d - j) << 27);
        for (int i = 0; i < RC_PACKED_SLOTS; ++i)
            if ((q[2 * i + 1] & cmask) != 0 && q[2 * i] == lo && (q[2 * i + 1] & mhi) == want) return false;
    }
    return true;
}

// table source: grid-stride over the buckets, each lane RC_SPEC_UNROLL whole buckets a step (a wavefront's load instruction
// covers 64 consecutive buckets, 2 KB), the slots decoded in registers; the live rule is rc_table_slot_entry's
__global__ __launch_bounds__(RC_SPEC_THREADS) void k_spectrum_table(rc_table_view T, uint32_t max_bin, uint32_t lds_bins,
                                                                     unsigned long long *__restrict__ out)
{
    __shared__ uint32_t s_small[RC_SPEC_WAVES * RC_SPEC_SMALL];
    extern __shared__ uint32_t s_big[];
    rc_spec_zero(s_small, s_big, lds_bins);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t *s_wave = s_small + w * RC_SPEC_SMALL;
    rc_spec_acc A;
    const size_t nb = T.nbuckets_alloc, per_wave = 64 * RC_SPEC_UNROLL;
    const size_t stride = (size_t)gridDim.x * RC_SPEC_WAVES * per_wave;
    const uint32_t cmask = RC_PACKED_COUNT_MASK >> T.ext;
    const uint32_t mhi = 0x7FFFFFFFu & ~cmask;  // remainder bits above the count, displacement
    for (size_t base = ((size_t)blockIdx.x * RC_SPEC_WAVES + w) * per_wave; base < nb; base += stride) {
        uint4 v[RC_SPEC_UNROLL][2];
#pragma unroll
        for (int u = 0; u < RC_SPEC_UNROLL; ++u) {
            const size_t b = base + (size_t)u * 64 + lane;
            v[u][0] = v[u][1] = make_uint4(0, 0, 0, 0);  // (beyond the table: no count in any slot of either layout)
            if (b < nb) {
                const uint4 *p = reinterpret_cast<const uint4 *>(T.buckets + b * RC_BUCKET_DWORDS);
                v[u][0] = p[0];
                v[u][1] = p[1];
            }
        }
#pragma unroll
        for (int u = 0; u < RC_SPEC_UNROLL; ++u) {
            const size_t b = base + (size_t)u * 64 + lane;
            const uint32_t d[8] = {v[u][0].x, v[u][0].y, v[u][0].z, v[u][0].w, v[u][1].x, v[u][1].y, v[u][1].z, v[u][1].w};
#ifdef RC_EXP_SPEC_LOAD_ONLY  // dev (WRONG spectrum): the bucket reads alone -- what the access pattern costs (tools/spectrum_time.py)
            A.total += d[0] ^ d[1] ^ d[2] ^ d[3] ^ d[4] ^ d[5] ^ d[6] ^ d[7];
            continue;
#endif
            if (T.layout) {
#pragma unroll
                for (int s = 0; s < RC_PACKED_SLOTS; ++s) {
                    const uint32_t lo = d[2 * s], hi = d[2 * s + 1];
                    uint32_t c = hi & cmask;
                    bool live = c != 0;
#pragma unroll
                    for (int i = 0; i < s; ++i)
                        if ((d[2 * i + 1] & cmask) != 0 && d[2 * i] == lo && ((d[2 * i + 1] ^ hi) & mhi) == 0) live = false;
#ifndef RC_EXP_SPEC_NO_WALK  // dev (WRONG for tables with duplicate keys): without the walk over the buckets in front
                    if (live && ((hi >> 27) & 15u)) live = rc_spec_packed_first(T, b, lo, hi, cmask, mhi);
#endif
                    if (live && c == cmask) {  // (rare) the full count lives in the table's prefix
                        const uint32_t disp = (hi >> 27) & 15u;
                        const uint64_t kk = rc_packed_key((uint32_t)(b - disp), lo, (hi & RC_PACKED_COUNT_MASK) >> (27 - T.ext), T.ext, T.k, T.nb_home);
                        c = (uint32_t)rc_packed_overflow_count(T, kk);
                    }
                    rc_spec_add(A, live, c, max_bin, lds_bins, s_wave, s_big, out);
                }
            } else {
#pragma unroll
                for (int s = 0; s < RC_WIDE_SLOTS; ++s) {
                    const uint32_t c = d[3 * s + 2];
                    bool live = c != 0;
                    if (live) {
                        const uint64_t kk = ((uint64_t)d[3 * s + 1] << 32) | d[3 * s];
                        if (rc_home(kk, T.nb_home) == b) {  // the walk starts here: an earlier slot of this bucket with the same key wins
#pragma unroll
                            for (int i = 0; i < s; ++i)
                                if (d[3 * i + 2] != 0 && d[3 * i] == d[3 * s] && d[3 * i + 1] == d[3 * s + 1]) live = false;
                        } else {  // (displaced: the walk from the key's home, in memory)
                            uint64_t key;
                            int32_t cc;
                            live = rc_table_slot_entry(T, b, s, &key, &cc);
                        }
                    }
                    rc_spec_add(A, live, c, max_bin, lds_bins, s_wave, s_big, out);
                }
            }
        }
    }
    rc_spec_flush(A, max_bin, lds_bins, s_small, s_big, out);
}

// counted source: the run-length counts of one key slice (what k_flag_keep filters), four per lane and step
__global__ __launch_bounds__(RC_SPEC_THREADS) void k_spectrum_counts(const uint32_t *__restrict__ cnt, size_t n, uint32_t max_bin, uint32_t lds_bins,
                                                                      unsigned long long *__restrict__ out)
{
    __shared__ uint32_t s_small[RC_SPEC_WAVES * RC_SPEC_SMALL];
    extern __shared__ uint32_t s_big[];
    rc_spec_zero(s_small, s_big, lds_bins);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t *s_wave = s_small + w * RC_SPEC_SMALL;
    rc_spec_acc A;
    const size_t nq = (n + 3) / 4, stride = (size_t)gridDim.x * RC_SPEC_WAVES * 64;
    for (size_t base = ((size_t)blockIdx.x * RC_SPEC_WAVES + w) * 64; base < nq; base += stride) {
        const size_t q = base + lane;
        uint32_t c[4] = {0, 0, 0, 0};
        if (q * 4 + 4 <= n) {
            const uint4 x = reinterpret_cast<const uint4 *>(cnt)[q];
            c[0] = x.x;
            c[1] = x.y;
            c[2] = x.z;
            c[3] = x.w;
        } else {
            for (int j = 0; j < 4; ++j)
                if (q * 4 + j < n) c[j] = cnt[q * 4 + j];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) rc_spec_add(A, c[j] != 0, c[j], max_bin, lds_bins, s_wave, s_big, out);
    }
    rc_spec_flush(A, max_bin, lds_bins, s_small, s_big, out);
}

static hipError_t rc_spec_allow_lds(const void *fn, size_t bytes)
{
    const size_t total = bytes + RC_SPEC_WAVES * RC_SPEC_SMALL * 4 + RC_SPEC_WAVES * 4 * 8;
    if (total <= 65536) return hipSuccess;
    return hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// d_out: max_bin + 1 + 4 uint64, zeroed by the caller before the first launch; adds one slice's counts (stream st)
int rc_launch_spectrum_counts(rc_ctx *ctx, hipStream_t st, const uint32_t *d_cnt, size_t n, uint32_t max_bin, unsigned long long *d_out)
{
    if (n == 0) return RC_OK;
    if (reinterpret_cast<uintptr_t>(d_cnt) & 15u) {
        rc_set_error(ctx, "spectrum: run-length counts not 16-byte aligned");
        return RC_ERR_ARG;
    }
    const uint32_t lds = rc_spec_lds_bins(max_bin);
    const size_t bytes = rc_spec_lds_bytes(lds);
    RC_CHECK_HIP(ctx, rc_spec_allow_lds(reinterpret_cast<const void *>(k_spectrum_counts), bytes));
    const size_t per_block = (size_t)RC_SPEC_WAVES * 64 * 4;
    const unsigned G = (unsigned)std::min<size_t>(RC_SPEC_MAX_BLOCKS, (n + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_spectrum_counts, dim3(G), dim3(RC_SPEC_THREADS), bytes, st, d_cnt, n, max_bin, lds, d_out);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// the spectrum of the context's table into host arrays freq[max_bin + 1], st[4]
int rc_table_spectrum_scan(rc_ctx *ctx, uint32_t max_bin, uint64_t *freq, uint64_t *st)
{
    const size_t words = (size_t)max_bin + 1 + 4;
    rc_dev_tmp b_out;
    RC_CHECK_HIP(ctx, b_out.alloc(words * 8));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_out.p, 0, words * 8, ctx->stream));
    const size_t nb = ctx->nb_alloc;
    if (nb) {
        const uint32_t lds = rc_spec_lds_bins(max_bin);
        const size_t bytes = rc_spec_lds_bytes(lds);
        RC_CHECK_HIP(ctx, rc_spec_allow_lds(reinterpret_cast<const void *>(k_spectrum_table), bytes));
        const size_t per_block = (size_t)RC_SPEC_WAVES * 64 * RC_SPEC_UNROLL;
        const unsigned G = (unsigned)std::min<size_t>(RC_SPEC_MAX_BLOCKS, (nb + per_block - 1) / per_block);
        hipLaunchKernelGGL(k_spectrum_table, dim3(G), dim3(RC_SPEC_THREADS), bytes, ctx->stream, rc_view(ctx), max_bin, lds,
                           b_out.as<unsigned long long>());
        RC_CHECK_HIP(ctx, hipGetLastError());
    }
    RC_CHECK_HIP(ctx, hipMemcpyAsync(freq, b_out.p, ((size_t)max_bin + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(st, b_out.as<unsigned long long>() + (size_t)max_bin + 1, 32, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RC_OK;
}

// ---- census of a recount session (rc_count.hip: rc_recount_finish_session hands every sorted slice to it) ---------------------
#define RC_CENSUS_UNROLL 2

// Per lane one distinct canonical code of a sorted slice and its count: is the code in the table (GetCount != 0), and the
// count into the spectrum (rc_spec_add, as k_spectrum_counts).  The codes are sorted by value, the table is addressed by
// hash, so every probe is a scattered 64-byte bucket read.  What round 6 learnt about such reads (docs/rounds/r6.md,
// tools/microbench_bucket.hip): their cost is the number of load INSTRUCTIONS times the lines each touches, not the bytes
// -- so the probe is rc_table_lookup_quad (a quad reads a bucket together: four instructions of 16 lines for four buckets
// instead of four of 64), and a lane keeps RC_CENSUS_UNROLL codes, eight such loads, in flight: with 16 waves a CU that is
// 128 outstanding instructions, where the microbenchmark's rate out of a table beyond the L2 no longer rose.
// out = freq[max_bin + 1], {distinct, total, unique, max_count}, {absent_distinct, absent_total}
__global__ __launch_bounds__(RC_SPEC_THREADS) void k_census(rc_table_view T, const uint64_t *__restrict__ uniq, const uint32_t *__restrict__ cnt, size_t n,
                                                            uint32_t max_bin, uint32_t lds_bins, unsigned long long *__restrict__ out)
{
    __shared__ uint32_t s_small[RC_SPEC_WAVES * RC_SPEC_SMALL];
    extern __shared__ uint32_t s_big[];
    rc_spec_zero(s_small, s_big, lds_bins);
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    uint32_t *s_wave = s_small + w * RC_SPEC_SMALL;
    rc_spec_acc A;
    unsigned long long absent_distinct = 0;  // wave-uniform (ballot counts)
    unsigned long long absent_total = 0;     // per lane
    const size_t per_wave = 64 * RC_CENSUS_UNROLL, stride = (size_t)gridDim.x * RC_SPEC_WAVES * per_wave;
    for (size_t base = ((size_t)blockIdx.x * RC_SPEC_WAVES + w) * per_wave; base < n; base += stride) {  // (wave-uniform: the quad lookup wants every lane)
        uint64_t key[RC_CENSUS_UNROLL];
        uint32_t c[RC_CENSUS_UNROLL];
        int in_table[RC_CENSUS_UNROLL];
#pragma unroll
        for (int u = 0; u < RC_CENSUS_UNROLL; ++u) {
            const size_t i = base + (size_t)u * 64 + lane;
            key[u] = i < n ? uniq[i] : 0;
            c[u] = i < n ? cnt[i] : 0;  // (a run length is at least 1: 0 = no code for this lane)
        }
#pragma unroll
        for (int u = 0; u < RC_CENSUS_UNROLL; ++u) in_table[u] = rc_table_lookup_quad<true>(T, key[u], c[u] != 0);
#pragma unroll
        for (int u = 0; u < RC_CENSUS_UNROLL; ++u) {
            const bool valid = c[u] != 0, absent = valid && in_table[u] == 0;
            rc_spec_add(A, valid, c[u], max_bin, lds_bins, s_wave, s_big, out);
            absent_distinct += (unsigned long long)__popcll(__ballot(absent));
            if (absent) absent_total += c[u];
        }
    }
    for (int o = 32; o > 0; o >>= 1) absent_total += __shfl_xor(absent_total, o, 64);
    if (lane == 0 && absent_distinct) {  // one atomic per wavefront and quantity
        atomicAdd(&out[(size_t)max_bin + 5], absent_distinct);
        atomicAdd(&out[(size_t)max_bin + 6], absent_total);
    }
    rc_spec_flush(A, max_bin, lds_bins, s_small, s_big, out);
}

// d_out: max_bin + 1 + 6 uint64, zeroed by the caller before the first launch; adds one slice (stream st)
int rc_launch_census(rc_ctx *ctx, hipStream_t st, const uint64_t *d_uniq, const uint32_t *d_cnt, size_t n, uint32_t max_bin, unsigned long long *d_out)
{
    if (n == 0) return RC_OK;
    const uint32_t lds = rc_spec_lds_bins(max_bin);
    const size_t bytes = rc_spec_lds_bytes(lds);
    RC_CHECK_HIP(ctx, rc_spec_allow_lds(reinterpret_cast<const void *>(k_census), bytes));
    const size_t per_block = (size_t)RC_SPEC_WAVES * 64 * RC_CENSUS_UNROLL;
    const unsigned G = (unsigned)std::min<size_t>(RC_SPEC_MAX_BLOCKS, (n + per_block - 1) / per_block);
    hipLaunchKernelGGL(k_census, dim3(G), dim3(RC_SPEC_THREADS), bytes, st, rc_view(ctx), d_uniq, d_cnt, n, max_bin, lds, d_out);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

__global__ void k_dump_order_keys(const uint64_t *__restrict__ codes, size_t n, uint64_t *__restrict__ keys)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) keys[i] = rc_dump_order_key(codes[i]);
}

// every (canonical code, count) of the table in dump order (rc_common.h: rc_dump_order_key), to host
int rc_table_entries_in_dump_order(rc_ctx *ctx, std::vector<uint64_t> *codes, std::vector<int32_t> *counts)
{
    const size_t cap = (size_t)ctx->n_entries;  // upper bound (duplicates were counted in)
    codes->clear();
    if (counts) counts->clear();
    if (cap == 0) return RC_OK;
    rc_dev_tmp b_codes, b_counts, b_n, b_keys, b_keys_s, b_codes_s, b_counts_s, b_tmp;
    unsigned long long n64 = 0;
    RC_CHECK_HIP(ctx, b_codes.alloc(cap * 8));
    RC_CHECK_HIP(ctx, b_counts.alloc(cap * 4));
    RC_CHECK_HIP(ctx, b_n.alloc(8));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_n.p, 0, 8, ctx->stream));
    int rc = rc_launch_export(ctx, b_codes.as<uint64_t>(), b_counts.as<int32_t>(), b_n.as<unsigned long long>(), cap);
    if (rc) return rc;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(&n64, b_n.p, 8, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (n64 > cap) {
        rc_set_error(ctx, "table export: %llu entries found, at most %zu expected", n64, cap);
        return RC_ERR_STATE;
    }
    const size_t n = (size_t)n64;
    codes->resize(n);
    if (counts) counts->resize(n);
    if (n == 0) return RC_OK;
    RC_CHECK_HIP(ctx, b_keys.alloc(n * 8));
    RC_CHECK_HIP(ctx, b_keys_s.alloc(n * 8));
    RC_CHECK_HIP(ctx, b_codes_s.alloc(n * 8));
    hipLaunchKernelGGL(k_dump_order_keys, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, b_codes.as<uint64_t>(), n, b_keys.as<uint64_t>());
    RC_CHECK_HIP(ctx, hipGetLastError());
    size_t t1 = 0, t2 = 0;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t1, b_keys.as<uint64_t>(), b_keys_s.as<uint64_t>(), b_codes.as<uint64_t>(), b_codes_s.as<uint64_t>(), n, 0, 64, ctx->stream));
    RC_CHECK_HIP(ctx, b_tmp.alloc(t1));
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(b_tmp.p, t1, b_keys.as<uint64_t>(), b_keys_s.as<uint64_t>(), b_codes.as<uint64_t>(), b_codes_s.as<uint64_t>(), n, 0, 64, ctx->stream));
    RC_CHECK_HIP(ctx, hipMemcpyAsync(codes->data(), b_codes_s.p, n * 8, hipMemcpyDeviceToHost, ctx->stream));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (counts) {
        RC_CHECK_HIP(ctx, b_counts_s.alloc(n * 4));
        RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t2, b_keys.as<uint64_t>(), b_keys_s.as<uint64_t>(), b_counts.as<int32_t>(), b_counts_s.as<int32_t>(), n, 0, 64, ctx->stream));
        RC_CHECK_HIP(ctx, b_tmp.alloc(t2));
        RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(b_tmp.p, t2, b_keys.as<uint64_t>(), b_keys_s.as<uint64_t>(), b_counts.as<int32_t>(), b_counts_s.as<int32_t>(), n, 0, 64, ctx->stream));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(counts->data(), b_counts_s.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return RC_OK;
}

__global__ void k_selftest_bound(const int32_t *__restrict__ c, size_t n, double e, int32_t *__restrict__ oi, double *__restrict__ od)
{
    size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    oi[i] = rc_bound_i(c[i], e);
    od[i] = rc_bound_d(c[i], e);
}

int rc_launch_selftest_bound(rc_ctx *ctx, const int32_t *d_c, size_t n, double e, int32_t *d_oi, double *d_od)
{
    if (n == 0) return RC_OK;
    hipLaunchKernelGGL(k_selftest_bound, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, d_c, n, e, d_oi, d_od);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// Work lists by flag value, in one pass: section c (0 .. NS-1) of d_list, at d_list + c * stride, receives the indices
// i in [0, n) with d_flag[i] == first + c * step; d_count[c] = how many.  A 256-thread workgroup takes 4096 flags (16 per
// thread, one 16-byte load), scans its per-section counts (four 16-bit fields of one 64-bit word) and claims its stretch
// of every section with one atomic per section.  Within a section the indices ascend inside a workgroup's stretch; the
// stretches themselves land in the order the workgroups got there -- nothing downstream depends on the order of a list
// (a read's result depends on its unit alone), only on which section a read is in.  [Rounds 2-3 ran one rocprim::select
// per section: 7 passes of ~0.24 ms over a batch's flags per step, each with its own lookback-scan initialisation.]
// values != nullptr: the lists receive values[i] instead of i (the length-tier lists: i = a position of the locality order,
// values[i] = the read there)
template <int NS>
__global__ __launch_bounds__(256) void k_compact_sections(const uint8_t *__restrict__ flag, uint32_t n, int first, int step,
                                                          uint32_t *__restrict__ list, size_t stride, uint32_t *__restrict__ count,
                                                          const uint32_t *__restrict__ values)
{
    static_assert(NS >= 1 && NS <= 4, "four 16-bit fields");
    __shared__ uint64_t s_wave[4];
    __shared__ uint32_t s_base[NS];
    const uint32_t t = threadIdx.x, lane = t & 63u, wave = t >> 6;
    for (uint32_t b0 = blockIdx.x * 4096u; b0 < n; b0 += gridDim.x * 4096u) {
        const uint32_t i0 = b0 + t * 16u;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (i0 < n) v = *reinterpret_cast<const uint4 *>(flag + i0);  // (the flag arrays are reserved with 256 bytes of slack)
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
        uint64_t mine = 0;  // field c = how many of this thread's flags belong to section c
        if (i0 < n && (v.x | v.y | v.z | v.w)) {
#pragma unroll
            for (int q = 0; q < 16; ++q) {
                const int f = (int)((w[q >> 2] >> (8 * (q & 3))) & 0xffu);
                if (i0 + q < n && f) {
#pragma unroll
                    for (int c = 0; c < NS; ++c) mine += f == first + c * step ? (1ull << (16 * c)) : 0ull;
                }
            }
        }
        // exclusive scan over the workgroup
        uint64_t inc = mine;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint64_t y = __shfl_up(inc, o, 64);
            inc += lane >= (uint32_t)o ? y : 0ull;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint64_t before = 0, total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            before += (uint32_t)q < wave ? s_wave[q] : 0ull;
            total += s_wave[q];
        }
        if (total) {  // (uniform)
            if (t < (uint32_t)NS) {
                const uint32_t c = (uint32_t)((total >> (16 * t)) & 0xffffu);
                s_base[t] = c ? atomicAdd(count + t, c) : 0u;
            }
            __syncthreads();
            if (mine) {
                const uint64_t ex = before + inc - mine;
                uint32_t pos[NS];
#pragma unroll
                for (int c = 0; c < NS; ++c) pos[c] = s_base[c] + (uint32_t)((ex >> (16 * c)) & 0xffffu);
#pragma unroll
                for (int q = 0; q < 16; ++q) {
                    const int f = (int)((w[q >> 2] >> (8 * (q & 3))) & 0xffu);
                    if (i0 + q < n && f) {
#pragma unroll
                        for (int c = 0; c < NS; ++c)
                            if (f == first + c * step) list[(size_t)c * stride + pos[c]++] = values ? values[i0 + (uint32_t)q] : i0 + (uint32_t)q;
                    }
                }
            }
        }
        __syncthreads();  // s_wave / s_base are rewritten by the next stretch
    }
}

template <int NS>
static int rc_compact_sections(rc_ctx *ctx, const uint8_t *d_flag, uint32_t n, int first, int step, uint32_t *d_list, size_t stride, uint32_t *d_count,
                               const uint32_t *d_values = nullptr, hipStream_t st = nullptr)
{
    if (!st) st = ctx->stream;
    RC_CHECK_HIP(ctx, hipMemsetAsync(d_count, 0, NS * sizeof(uint32_t), st));
    if (n == 0) return RC_OK;
    unsigned grid = (n + 4095u) / 4096u;
    if (grid > (unsigned)ctx->n_cu * 32u) grid = (unsigned)ctx->n_cu * 32u;
    hipLaunchKernelGGL(k_compact_sections<NS>, dim3(grid), dim3(256), 0, st, d_flag, n, first, step, d_list, stride, d_count, d_values);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// section c (0 .. RC_WORK_CLASSES-1) of d_list = the reads with d_cls[i] == RC_WORK_CLASSES - c (k_correct's list: the
// classes expected to be expensive first)
int rc_launch_compact(rc_ctx *ctx, const uint8_t *d_cls, uint32_t n, uint32_t *d_list, size_t stride, uint32_t *d_count)
{
    return rc_compact_sections<RC_WORK_CLASSES>(ctx, d_cls, n, RC_WORK_CLASSES, -1, d_list, stride, d_count);
}

// the same with every section in the batch's locality order (RC_K3_LOCAL=1, dev): the classes are gathered through the order
// (ctx->loc_list: every read once) and the compaction hands out the list's entries instead of positions
__global__ __launch_bounds__(256) void k_gather_u8(const uint8_t *__restrict__ src, const uint32_t *__restrict__ idx, uint32_t n, uint8_t *__restrict__ dst)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) dst[i] = src[idx[i]];
}
int rc_launch_compact_local(rc_ctx *ctx, const uint8_t *d_cls, uint32_t n, uint32_t *d_list, size_t stride, uint32_t *d_count)
{
    int rc = rc_dbuf_reserve(ctx, &ctx->tier_flag, (size_t)n + 256);  // (the tiers' flag array: free at this point of a pass)
    if (rc) return rc;
    hipLaunchKernelGGL(k_gather_u8, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_cls, (const uint32_t *)ctx->loc_list.p, n, (uint8_t *)ctx->tier_flag.p);
    return rc_compact_sections<RC_WORK_CLASSES>(ctx, (const uint8_t *)ctx->tier_flag.p, n, RC_WORK_CLASSES, -1, d_list, stride, d_count, (const uint32_t *)ctx->loc_list.p);
}

// The chunked pipeline's compactions (rc_correct_device_impl): positions [lo, hi) of the locality order alone.  The flags of the
// reads there are gathered through the order into ctx->tier_flag (free: no length tiers where the pipeline runs; at most one
// compaction is in flight, the follower stream being serial) and compacted with the order's entries as values, as above.
template <int NS>
static int rc_compact_range(rc_ctx *ctx, hipStream_t st, const uint8_t *d_flag, uint32_t lo, uint32_t hi, int first, int step, uint32_t *d_list, size_t stride,
                            uint32_t *d_count)
{
    const uint32_t m = hi > lo ? hi - lo : 0;
    int rc = rc_dbuf_reserve(ctx, &ctx->tier_flag, (size_t)m + 256);
    if (rc) return rc;
    const uint32_t *order = (const uint32_t *)ctx->loc_list.p + lo;
    if (m) hipLaunchKernelGGL(k_gather_u8, dim3((m + 255) / 256), dim3(256), 0, st, d_flag, order, m, (uint8_t *)ctx->tier_flag.p);
    return rc_compact_sections<NS>(ctx, (const uint8_t *)ctx->tier_flag.p, m, first, step, d_list, stride, d_count, order, st);
}
int rc_launch_compact_range(rc_ctx *ctx, hipStream_t st, const uint8_t *d_cls, uint32_t lo, uint32_t hi, uint32_t *d_list, size_t stride, uint32_t *d_count)
{
    return rc_compact_range<RC_WORK_CLASSES>(ctx, st, d_cls, lo, hi, RC_WORK_CLASSES, -1, d_list, stride, d_count);
}
int rc_launch_compact_flag_range(rc_ctx *ctx, hipStream_t st, const uint8_t *d_flag, uint32_t lo, uint32_t hi, uint32_t *d_list, size_t stride, uint32_t *d_count)
{
    return rc_compact_range<3>(ctx, st, d_flag, lo, hi, 1, 1, d_list, stride, d_count);
}

// section v - 1 (v = 1 .. 3) of d_list = the reads with d_flag[i] == v (k_single's list: by number of untrusted stretches)
int rc_launch_compact_flag(rc_ctx *ctx, const uint8_t *d_flag, uint32_t n, uint32_t *d_list, size_t stride, uint32_t *d_count)
{
    return rc_compact_sections<3>(ctx, d_flag, n, 1, 1, d_list, stride, d_count);
}

// ---- locality order of a batch -------------------------------------------------------------------
// Reads arrive in sequencer order, i.e. random with respect to the transcripts they come from, so the
// ~130 probes of a read hit ~130 unrelated buckets and nearly every one of them is an HBM access.
// Reads that overlap share most of their k-mers: probed next to each other, they meet in the L2 /
// Infinity Cache instead.  Large batches are therefore PROBED in "min-hash order": key of a unit (a
// read, or a pair through its first mate) = the smallest hash over its canonical m-mers (m = min(k, 16), see
// k_unit_key), so units that contain the same m-mer as their minimum -- overlapping reads -- become neighbours in the list
// k_probe_list walks.  Nothing is moved: counts land at the reads' own positions, and the threshold
// and correction kernels run as ever.
#define RC_KEY_TILE 40960  // bytes of reads staged per 256-thread workgroup of k_unit_key
__global__ __launch_bounds__(256) void k_unit_key(const uint8_t *__restrict__ seq, size_t nbytes, const uint32_t *__restrict__ off,
                                                  uint32_t n_units, int mode, int k, uint32_t units_per_block,
                                                  uint32_t *__restrict__ keys, uint32_t *__restrict__ idx)
{
    __shared__ __attribute__((aligned(16))) uint8_t s_raw[RC_KEY_TILE + 48];
    const uint32_t u0 = blockIdx.x * units_per_block;
    if (u0 >= n_units) return;
    const uint32_t nu = n_units - u0 < units_per_block ? n_units - u0 : units_per_block;
    const uint32_t r0 = mode == 2 ? 2u * u0 : u0, r1 = mode == 2 ? 2u * (u0 + nu) : u0 + nu;
    const size_t b0 = off[r0], b1 = off[r1], a0 = b0 & ~(size_t)15;
    // the tile's bytes, coalesced (a thread-per-read walk over global memory touches a line per lane per load)
    for (size_t c = threadIdx.x; a0 + 16 * c < b1; c += 256) {
        const size_t g = a0 + 16 * c;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (g + 16 <= nbytes) {
            v = *reinterpret_cast<const uint4 *>(seq + g);
        } else {
            uint32_t w[4] = {0, 0, 0, 0};
            for (size_t q = 0; g + q < nbytes; ++q) w[q >> 2] |= (uint32_t)seq[g + q] << (8 * (q & 3));
            v = make_uint4(w[0], w[1], w[2], w[3]);
        }
        *reinterpret_cast<uint4 *>(s_raw + 16 * c) = v;
    }
    __syncthreads();
    if (threadIdx.x >= nu) return;
    const uint32_t u = u0 + threadIdx.x;
    const uint32_t r = mode == 2 ? 2u * u : u;  // the unit's first mate
    const uint32_t o = (uint32_t)(off[r] - a0);
    const int len = (int)(off[r + 1] - off[r]) - 1;
    // The key only has to make overlapping reads neighbours, so it is the smallest hash over the read's canonical m-mers,
    // m = min(k, 16): two reads that overlap by m bases or more share their minimum whenever it lies in the overlap, as with
    // k-mers -- and an m-mer is one 32-bit word, which takes this loop (a thread per unit, bound by instruction issue) from
    // 64-bit shifts, compares and two more multiplies per base to a handful of 32-bit operations (RC_KEY_KMER=1 at compile
    // time keeps the k-mer version for A/B runs).
#ifndef RC_KEY_KMER
    const int m = k < 16 ? k : 16;
    const uint32_t mask = m == 16 ? 0xFFFFFFFFu : ((1u << (2 * m)) - 1u);
    const int top = 2 * (m - 1);
    uint32_t fw = 0, rv = 0, best = 0xFFFFFFFFu;
    int valid = 0;
#ifdef RC_KEY_OFFSET
    int best_i = 0;
    bool best_rev = false;
#endif
    for (int i = 0; i < len; ++i) {
        const uint32_t c = s_raw[o + i];
        const uint32_t b = ((c >> 1) ^ (c >> 2)) & 3u;                     // A 0, C 1, G 2, T 3
        const uint32_t d = c - 65u;                                        // 'A' .. 'T': bits 0, 2, 6, 19 of the mask
        const bool acgt = d < 20u && ((0x80045u >> d) & 1u);
        valid = acgt ? valid + 1 : 0;
        fw = ((fw << 2) | b) & mask;
        rv = (rv >> 2) | ((3u - b) << top);
        if (valid >= m) {
            uint32_t h = (fw < rv ? fw : rv) * 0x9E3779B1u;
            h ^= h >> 15;
            h *= 0x2C1B3C6Du;
            h ^= h >> 13;
#ifdef RC_KEY_OFFSET
            if (h < best) {
                best_i = i;
                best_rev = rv < fw;
            }
#endif
            best = h < best ? h : best;
        }
    }
#ifdef RC_KEY_OFFSET
    // Within a group of units that share their minimal m-mer, the order is that of the reads' starts in the frame in which
    // the m-mer is forward (its offset in the read, or in the read's reverse complement): neighbours in the list then
    // overlap in all but a few bases instead of two thirds of them, and a k-mer's second probe follows its first one a
    // read later instead of somewhere in the group -- inside what the L2 still holds.  Seven bits of the key, half a base each.
    if (best != 0xFFFFFFFFu) {
        int p = best_rev ? len - 1 - best_i : best_i - m + 1;
        p = (p >> 1) > 127 ? 127 : (p >> 1);
        best = (best & ~0x7Fu) | (uint32_t)(127 - p);  // (descending offset = ascending start)
    }
#endif
#else
    const uint64_t mask = rc_kmer_mask(k);
    uint64_t fw = 0, rv = 0;
    uint32_t best = 0xFFFFFFFFu;
    int valid = 0;
    for (int i = 0; i < len; ++i) {
        const uint32_t c = s_raw[o + i];
        int b = -1;
        b = c == 'A' ? 0 : b;
        b = c == 'C' ? 1 : b;
        b = c == 'G' ? 2 : b;
        b = c == 'T' ? 3 : b;
        valid = b < 0 ? 0 : valid + 1;
        fw = ((fw << 2) | (uint64_t)(b & 3)) & mask;
        rv = (rv >> 2) | ((uint64_t)(3 - (b & 3)) << (2 * (k - 1)));
        if (valid >= k) {
            const uint32_t h = rc_hash(fw < rv ? fw : rv);
            best = h < best ? h : best;
        }
    }
#endif
    keys[u] = best;
    idx[u] = u;
}

// list[i] = the reads in the order k_probe_list takes them: sorted units, the mates of a pair together
// span[i] (round 6) = where read list[i] lies in the arena -- {first byte, bytes with the NUL}: the fused probe kernel's workgroups
// then find their reads with two coalesced loads side by side instead of a load of the list and, behind it, a gather of the offsets
__global__ void k_probe_order(const uint32_t *__restrict__ unit_sorted, uint32_t n, int mode, uint32_t *__restrict__ list,
                              const uint32_t *__restrict__ off, uint2 *__restrict__ span)
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    uint32_t r;
    if (mode == 1)
        r = unit_sorted[i >> 1] + ((i & 1u) ? (n >> 1) : 0u);
    else if (mode == 2)
        r = 2u * unit_sorted[i >> 1] + (i & 1u);
    else
        r = unit_sorted[i];
    list[i] = r;
    const uint32_t g0 = off[r];
    span[i] = make_uint2(g0, off[r + 1] - g0);
}

int rc_launch_locality_order(rc_ctx *ctx, const rc_device_batch_args &a, size_t nbytes)
{
    const uint32_t n = a.n, n_units = a.mode ? n >> 1 : n;
    int rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->loc_a, (size_t)n_units * 16 + 256))) return rc;  // keys, keys', idx, idx'
    if ((rc = rc_dbuf_reserve(ctx, &ctx->loc_list, (size_t)n * 4 + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->loc_span, (size_t)n * 8 + 256))) return rc;
    uint32_t *keys = (uint32_t *)ctx->loc_a.p, *keys2 = keys + n_units, *idx = keys2 + n_units, *idx2 = idx + n_units;
    uint32_t upb = (uint32_t)(RC_KEY_TILE / ((size_t)(a.max_len + 1) * (a.mode == 2 ? 2 : 1)));
    if (upb > 256) upb = 256;
    if (upb < 1) upb = 1;
    hipLaunchKernelGGL(k_unit_key, dim3((n_units + upb - 1) / upb), dim3(256), 0, ctx->stream, a.seq, nbytes, a.off, n_units, a.mode, ctx->k, upb, keys, idx);
    size_t t1 = 0;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t1, keys, keys2, idx, idx2, (size_t)n_units, 0, 32, ctx->stream));
    if ((rc = rc_dbuf_reserve(ctx, &ctx->sel_tmp, t1))) return rc;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(ctx->sel_tmp.p, t1, keys, keys2, idx, idx2, (size_t)n_units, 0, 32, ctx->stream));
    hipLaunchKernelGGL(k_probe_order, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, idx2, n, a.mode, (uint32_t *)ctx->loc_list.p, a.off,
                       (uint2 *)ctx->loc_span.p);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// Length tiers of a mixed-length batch (rc_api_batch.hip: rc_correct_device_impl): flag of list position i = 0 if the unit of the read
// there -- the read, or the pair it is a mate of -- belongs to the short tier (its longer read has at most s_hi bases), 1 for
// the middle tier (at most m_hi), 2 for the long one.  Compacted, the positions of a tier give the reads of that tier in
// locality order, mates still adjacent: what the list-driven probe and threshold kernels of the tier's pass walk.
__global__ __launch_bounds__(256) void k_tier_flags(const uint32_t *__restrict__ off, const uint32_t *__restrict__ list, uint32_t n, int mode,
                                                    int s_hi, int m_hi, uint8_t *__restrict__ flag)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = list[i];
    int ml = (int)(off[r + 1] - off[r]) - 1;
    if (mode != 0) {
        const uint32_t half = n >> 1, mr = mode == 1 ? (r < half ? r + half : r - half) : (r ^ 1u);
        const int m1 = (int)(off[mr + 1] - off[mr]) - 1;
        ml = m1 > ml ? m1 : ml;
    }
    flag[i] = ml <= s_hi ? 0 : (ml <= m_hi ? 1 : 2);
}

// ctx->tier_list: two sections of `stride` entries (middle tier, long tier), their lengths at work + RC_WORK_NTIER_OFF
int rc_launch_tier_lists(rc_ctx *ctx, const rc_device_batch_args &a, int s_hi, int m_hi)
{
    int rc;
    const size_t stride = ((size_t)a.n + 63) & ~(size_t)63;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->tier_flag, (size_t)a.n + 256))) return rc;
    if ((rc = rc_dbuf_reserve(ctx, &ctx->tier_list, stride * 2 * 4 + 256))) return rc;
    ctx->tier_stride = stride;
    hipLaunchKernelGGL(k_tier_flags, dim3((a.n + 255) / 256), dim3(256), 0, ctx->stream, a.off, (const uint32_t *)ctx->loc_list.p, a.n, a.mode, s_hi, m_hi,
                       (uint8_t *)ctx->tier_flag.p);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return rc_compact_sections<2>(ctx, (const uint8_t *)ctx->tier_flag.p, a.n, 1, 1, (uint32_t *)ctx->tier_list.p, stride,
                                  (uint32_t *)((char *)ctx->work.p + RC_WORK_NTIER_OFF), (const uint32_t *)ctx->loc_list.p);
}

// ---- K1: probe kernel ----------------------------------------------------------------------
// counts[a] = GetCount(k-mer starting at arena byte a) for every a whose k-window lies inside one
// read (reads are NUL-terminated inside the arena, so "inside one read" == "no NUL in the
// window").  Windows holding a non-ACGT letter give 0 without touching the table (Store.h:61-62).
// One 256-thread workgroup owns a 4 KiB tile of the arena: it stages the tile (+32 B halo) into
// LDS as 2-bit codes plus two bit masks (non-ACGT, NUL; rc_device.h: rc_tile_stage), then every lane cuts
// its windows out of them (rc_common.h: rc_tile_window), canonicalises with bit-reverse and probes one bucket.
// seq is 16-byte aligned.
template <bool EXT>
__global__ __launch_bounds__(RC_PROBE_THREADS) void k_probe(rc_table_view T, const uint8_t *__restrict__ seq,
                                                            size_t nbytes, int k, int32_t *__restrict__ counts)
{
    __shared__ uint32_t s_code[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_inv[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_nul[RC_PROBE_TILE / 16 + 4];
    const size_t tile0 = (size_t)blockIdx.x * RC_PROBE_TILE;
    const int t = threadIdx.x;

    rc_tile_stage(seq, 0, nbytes, tile0, s_code, s_inv, s_nul);
    __syncthreads();
    const uint32_t *m_inv = reinterpret_cast<const uint32_t *>(s_inv);
    const uint32_t *m_nul = reinterpret_cast<const uint32_t *>(s_nul);

#pragma unroll 2
    for (int a = t; a < RC_PROBE_TILE; a += RC_PROBE_THREADS) {
        const size_t g = tile0 + (size_t)a;
        if (g + (size_t)k > nbytes) break;
        const rc_tile_win w = rc_tile_window(s_code, m_inv, m_nul, a, k);
        if (w.nul) continue;  // window crosses a read boundary: not a k-mer of any read
        const int cnt = w.bad ? 0 : rc_table_lookup<EXT>(T, rc_canonical(w.code, k));
        __builtin_nontemporal_store(cnt, &counts[g]);  // streamed once: keep it out of the caches the table lives in
    }
}

// K1 over a list of reads (locality order): the workgroup's reads are copied into a local arena in
// LDS (rc_device.h: rc_tile_copy_reads) -- each at the byte alignment it has in memory, NULs in between -- and that arena is
// k_probe's tile: the same planes (rc_tile_pack), the same window cut; a count goes to the position of its k-mer in the
// caller's arena.
// skip_hi >= 0: the reads of units (a read, or a pair: mode as in rc_kernel_args) whose longer read has at most skip_hi
// bases are left out -- the fused probe + threshold kernel of the short tier has their counts (rc_correct.hip).
template <bool EXT>
__global__ __launch_bounds__(RC_PROBE_THREADS) void k_probe_list(rc_table_view T, const uint8_t *__restrict__ seq, size_t nbytes,
                                                                 const uint32_t *__restrict__ off, const uint32_t *__restrict__ list,
                                                                 uint32_t n, uint32_t reads_per_block, int k, int32_t *__restrict__ counts,
                                                                 int mode, int skip_hi, const uint32_t *__restrict__ n_list)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_raw[(RC_PROBE_TILE + 64) / 4];
    __shared__ uint32_t s_code[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_inv[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_nul[RC_PROBE_TILE / 16 + 4];
    __shared__ uint32_t s_lpos[RC_PLIST_MAX_READS + 1], s_gpos[RC_PLIST_MAX_READS], s_len1[RC_PLIST_MAX_READS];
    const int t = threadIdx.x;
    // n_list != nullptr: `list` is a tier's list whose length lives on the device (rc_launch_tier_lists); a fixed grid walks it
    const uint32_t n_eff = n_list ? *n_list : n;
    for (uint32_t i0 = blockIdx.x * reads_per_block; i0 < n_eff; i0 += gridDim.x * reads_per_block) {
    const uint32_t nr = n_eff - i0 < reads_per_block ? n_eff - i0 : reads_per_block;
    bool any_live = false;
    if ((uint32_t)t < nr) {
        const uint32_t r = list[i0 + t], g0 = off[r];
        uint32_t len1 = off[r + 1] - g0;  // bases + the NUL
        if (skip_hi >= 0) {
            uint32_t ml1 = len1;
            if (mode != 0) {
                const uint32_t half = n >> 1, mr = mode == 1 ? (r < half ? r + half : r - half) : (r ^ 1u);
                const uint32_t m1 = off[mr + 1] - off[mr];
                ml1 = m1 > ml1 ? m1 : ml1;
            }
            if ((int)ml1 - 1 <= skip_hi) len1 = 0;  // 0 = not a read of this launch
        }
        s_gpos[t] = g0;
        s_len1[t] = len1;
        any_live = len1 != 0;
    }
    // (a mixed-length batch's short reads were probed by the fused kernel: most workgroups of this launch hold none)
    if (!__syncthreads_or(any_live)) continue;
    for (int c = t; c < (RC_PROBE_TILE + 64) / 4; c += RC_PROBE_THREADS) s_raw[c] = 0;
    if (t == 0) {  // local start of each read: same alignment modulo 4 as in memory, a NUL in front
        uint32_t lp = 4;
        for (uint32_t j = 0; j < nr; ++j) {
            lp = ((lp + 3u) & ~3u) + (s_gpos[j] & 3u);
            s_lpos[j] = lp;
            lp += s_len1[j];
        }
        s_lpos[nr] = lp;
    }
    __syncthreads();
    rc_tile_copy_reads<RC_PROBE_THREADS>(s_raw, s_gpos, s_lpos, s_len1, nr, seq, nbytes);
    __syncthreads();
    const uint32_t total = s_lpos[nr];
    for (int chunk = t; chunk < RC_PROBE_TILE / 16 + 2; chunk += RC_PROBE_THREADS)
        rc_tile_pack(*reinterpret_cast<const uint4 *>(s_raw + 4 * chunk), chunk, s_code, s_inv, s_nul);
    rc_tile_sentinels(s_code);
    __syncthreads();
    const uint32_t *m_inv = reinterpret_cast<const uint32_t *>(s_inv);
    const uint32_t *m_nul = reinterpret_cast<const uint32_t *>(s_nul);
#pragma unroll 2
    for (uint32_t a = 4 + (uint32_t)t; a + (uint32_t)k <= total; a += RC_PROBE_THREADS) {
        const rc_tile_win w = rc_tile_window(s_code, m_inv, m_nul, (int)a, k);
        if (w.nul) continue;  // window crosses a read boundary (or padding)
        const int cnt = w.bad ? 0 : rc_table_lookup<EXT>(T, rc_canonical(w.code, k));
        // the read this position belongs to: last j with lpos[j] <= a
        uint32_t lo = 0, hi = nr;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_lpos[mid] <= a)
                lo = mid;
            else
                hi = mid;
        }
        __builtin_nontemporal_store(cnt, &counts[s_gpos[lo] + (a - s_lpos[lo])]);
    }
    __syncthreads();  // (the next stretch of the list rewrites the tile)
    }
}

// reads per workgroup of k_probe_list: a read takes its bases, the NUL and up to 6 bytes of alignment
static uint32_t rc_probe_list_rpb(int max_len)
{
    const uint32_t rpb = (uint32_t)((RC_PROBE_TILE - 8) / (max_len + 8));
    return rpb > RC_PLIST_MAX_READS ? RC_PLIST_MAX_READS : (rpb < 1 ? 1 : rpb);
}

int rc_launch_probe_list(rc_ctx *ctx, const rc_device_batch_args &a, size_t nbytes, int32_t *d_counts, int skip_hi)
{
    if (a.n == 0) return RC_OK;
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "probe: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    const uint32_t rpb = rc_probe_list_rpb(a.max_len);
    rc_timer_begin(ctx);
    rc_with_ext(ctx->ext, [&](auto ext) {
        hipLaunchKernelGGL(k_probe_list<decltype(ext)::value>, dim3((a.n + rpb - 1) / rpb), dim3(RC_PROBE_THREADS), 0, ctx->stream, rc_view(ctx), a.seq, nbytes,
                           a.off, (const uint32_t *)ctx->loc_list.p, a.n, rpb, ctx->k, d_counts, a.mode, skip_hi, (const uint32_t *)nullptr);
    });
    rc_timer_end(ctx, RC_T_PROBE);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

int rc_launch_probe_tier(rc_ctx *ctx, const rc_device_batch_args &a, size_t nbytes, int32_t *d_counts, int section)
{
    if (a.n == 0) return RC_OK;
    const uint32_t rpb = rc_probe_list_rpb(a.max_len);
    const uint32_t *list = (const uint32_t *)ctx->tier_list.p + (size_t)section * ctx->tier_stride;
    const uint32_t *n_list = (const uint32_t *)((char *)ctx->work.p + RC_WORK_NTIER_OFF) + section;
    unsigned grid = (a.n + rpb - 1) / rpb;  // (at most: the tier's share of the batch is not known here)
    if (grid > (unsigned)ctx->n_cu * 16u) grid = (unsigned)ctx->n_cu * 16u;
    rc_timer_begin(ctx);
    rc_with_ext(ctx->ext, [&](auto ext) {
        hipLaunchKernelGGL(k_probe_list<decltype(ext)::value>, dim3(grid), dim3(RC_PROBE_THREADS), 0, ctx->stream, rc_view(ctx), a.seq, nbytes, a.off, list,
                           a.n, rpb, ctx->k, d_counts, a.mode, -1, n_list);
    });
    rc_timer_end(ctx, RC_T_PROBE);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

int rc_launch_probe(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, int32_t *d_counts)
{
    if (nbytes == 0) return RC_OK;
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "probe: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    const unsigned G = (unsigned)((nbytes + RC_PROBE_TILE - 1) / RC_PROBE_TILE);
    rc_timer_begin(ctx);
    rc_with_ext(ctx->ext, [&](auto ext) {
        hipLaunchKernelGGL(k_probe<decltype(ext)::value>, dim3(G), dim3(RC_PROBE_THREADS), 0, ctx->stream, rc_view(ctx), d_seq, nbytes, ctx->k, d_counts);
    });
    rc_timer_end(ctx, RC_T_PROBE);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
