// rc_recur.hip -- the recurrent-correction census (include/rcorrector_amd.h: rc_recur_census; the keys' arithmetic in
// rc_recur.h): one 61-bit site key per contexted change of a batch, and the census of a key array -- how many distinct sites,
// how many of them were corrected c times, and the sites corrected most often.
//
// k_change_keys: the streaming comparison of rc_report.hip -- a quarter wave (16 lanes) per read, 16 bytes per lane and step,
// both arenas read in ALIGNED 16-byte pieces (the snapshot has the arena's alignment modulo 16) with the bytes outside the
// read masked off, a bounded number of persistent workgroups striding over the reads.  Changes are sparse (about 1 % of the
// bases), so only a lane that holds a differing byte goes on: where the 29-byte window lies inside the read it fetches the two
// or three aligned pieces that hold it from the CORRECTED arena, shifts them together, packs them sixteen bytes at a time
// (rc_pack16m) and canonicalises on the packed word.  The keys are appended with one atomic per wavefront and round (ballot,
// popcount prefix) -- into a stage of the workgroup in LDS, which goes out to `keys` with ONE global atomic once it is half full:
// at 0.75 changes per read a round of a wavefront holds a key or two, and one global atomic per round, fifteen million to one
// address per batch of the benchmark's shard, took 75 ms where the comparison takes three.  Nothing is written past `cap`; the
// cursor counts every key all the same, so a caller whose buffer was too small learns how much it needs.  A piece that holds a
// byte of the arena lies in that byte's page: the loads up to 15 bytes outside it cannot fault, and what they bring never
// passes the mask.
//
// The census: a 64-bit radix sort of a copy of the keys, a run-length encode, a histogram of the run lengths (LDS for the small
// bins, where nearly all runs are), and for the top list a stable sort of the runs by descending length -- the runs come out
// of the encode in ascending key order, which the stable sort keeps among equal lengths.
#include <algorithm>
#include <cstring>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "rc_internal.h"
#include "rc_device.h"
#include "rc_recur.h"

#define RC_RECUR_THREADS 256
#define RC_RECUR_QUARTERS (RC_RECUR_THREADS / 16)
#define RC_RECUR_STAGE 1024  // keys a workgroup stages in LDS before they go out together

typedef unsigned __int128 rc_u128;
__device__ __forceinline__ rc_u128 rc_recur_u128(const uint4 &p)
{
    return ((rc_u128)(((uint64_t)p.w << 32) | p.z) << 64) | (((uint64_t)p.y << 32) | p.x);
}

// the window whose first byte is at ws, all of it inside the corrected read: packed into *w; false: a byte outside ACGT
__device__ __forceinline__ bool rc_recur_fetch(const uint8_t *ws, uint64_t *w)
{
    const uintptr_t a0 = (uintptr_t)ws & ~(uintptr_t)15;
    const uint32_t sh = (uint32_t)((uintptr_t)ws - a0);
    const uint4 *pc = reinterpret_cast<const uint4 *>(a0);
    const uint4 p0 = pc[0], p1 = pc[1];  // (bytes [0, 16 - sh) and [16 - sh, 29) of the window: both hold some)
    uint4 p2 = make_uint4(0, 0, 0, 0);
    if (sh + (uint32_t)RC_RECUR_WINDOW > 32u) p2 = pc[2];  // (holds one too)
    const rc_u128 x0 = rc_recur_u128(p0), x1 = rc_recur_u128(p1), x2 = rc_recur_u128(p2);
    const rc_u128 lo = sh ? (x0 >> (8u * sh)) | (x1 << (128u - 8u * sh)) : x0;
    const rc_u128 hi = sh ? (x1 >> (8u * sh)) | (x2 << (128u - 8u * sh)) : x1;
    const uint32_t d[8] = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)(lo >> 64), (uint32_t)(lo >> 96),
                           (uint32_t)hi, (uint32_t)(hi >> 32), (uint32_t)(hi >> 64), (uint32_t)(hi >> 96)};
    return rc_recur_window(d, w);
}

// after: the corrected arena, nbytes of it; the arena as it arrived has its byte p at after + p + delta (a multiple of 16);
// off[n + 1]; keys[cap]; counts[3] = changes, contexted changes, keys appended (the cursor: it passes cap where they do not fit)
__global__ __launch_bounds__(RC_RECUR_THREADS) void k_change_keys(const uint8_t *__restrict__ after, ptrdiff_t delta, const uint32_t *__restrict__ off, uint32_t n,
                                                                  uint32_t nbytes, uint64_t *__restrict__ keys, unsigned long long cap,
                                                                  unsigned long long *__restrict__ counts)
{
    __shared__ uint64_t s_key[RC_RECUR_STAGE];
    __shared__ uint32_t s_tot[2], s_n;
    __shared__ unsigned long long s_base;
    if (threadIdx.x < 2) s_tot[threadIdx.x] = 0;
    if (threadIdx.x == 0) s_n = 0;
    __syncthreads();
    // called by the whole workgroup, all keys staged: the stage appended to `keys` (never past cap; the cursor counts them all)
    auto flush = [&]() {
        const uint32_t n_st = s_n < RC_RECUR_STAGE ? s_n : RC_RECUR_STAGE;  // (slots reserved past the stage went out directly)
        if (threadIdx.x == 0) s_base = atomicAdd(&counts[2], (unsigned long long)n_st);
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < n_st; i += RC_RECUR_THREADS) {
            const unsigned long long at = s_base + i;
            if (at < cap) keys[at] = s_key[i];
        }
        __syncthreads();
        if (threadIdx.x == 0) s_n = 0;
        __syncthreads();
    };
    const uint32_t l16 = threadIdx.x & 15u, lane = threadIdx.x & 63u;
    const uint32_t n_quarters = gridDim.x * RC_RECUR_QUARTERS, q = blockIdx.x * RC_RECUR_QUARTERS + (threadIdx.x >> 4);
    const uint32_t iters = (n + n_quarters - 1) / n_quarters;  // (the same for every lane: the ballots below want whole wavefronts)
    uint32_t my_changes = 0, my_keys = 0;
    bool over = false;
    uint64_t over_key = 0;
    for (uint32_t it = 0; it < iters; ++it) {
        const uint64_t r = (uint64_t)q + (uint64_t)it * n_quarters;  // (64 bits: the last stride may pass 2^32)
        uint32_t o = 0, len = 0;
        if (r < n) {
            o = off[r];
            const uint32_t o1 = off[r + 1];
            // (offsets ascend and end inside the arena by contract; ones that do not must still not send a load outside it)
            if (o > nbytes) o = nbytes;
            const uint32_t e = o1 > nbytes ? nbytes : o1;
            len = e > o ? e - o - 1u : 0u;
        }
        // aligned 16-byte pieces [a0 + 16 c, ...) that cover the read's bytes [s, s + len)
        const uint8_t *rd = after + o;
        const uintptr_t s = (uintptr_t)rd, a0 = s & ~(uintptr_t)15;
        const uint32_t lead = (uint32_t)(s - a0), n_pc = len ? (lead + len + 15u) >> 4 : 0u;
        for (uint32_t c = l16; __any(c < n_pc); c += 16) {  // (every lane of the wavefront stays in the loop until all are done)
            uint32_t d = 0;
            uint4 sv = make_uint4(0, 0, 0, 0), ov = sv;
            if (c < n_pc) {
                const uint8_t *pa = reinterpret_cast<const uint8_t *>(a0 + (uintptr_t)16 * c);
                sv = *reinterpret_cast<const uint4 *>(pa);
                ov = *reinterpret_cast<const uint4 *>(pa + delta);
            }
            const uint32_t sw[4] = {sv.x, sv.y, sv.z, sv.w}, ow[4] = {ov.x, ov.y, ov.z, ov.w};
            // the bytes of the piece that are this read's: position 0 of the read is byte lead - 16 c of the piece
            const int first = (int)lead - (int)(16u * c);
            if ((sw[0] ^ ow[0]) | (sw[1] ^ ow[1]) | (sw[2] ^ ow[2]) | (sw[3] ^ ow[3])) {  // (most pieces hold no change)
#pragma unroll
                for (int j = 0; j < 16; ++j) d |= ((((sw[j >> 2] ^ ow[j >> 2]) >> (8 * (j & 3))) & 0xffu) ? 1u : 0u) << j;
                const int last = first + (int)len;  // [first, last) within the piece, last > 0
                const uint32_t lo = first > 0 ? (uint32_t)first : 0u, hi = last < 16 ? (uint32_t)last : 16u;
                d &= (0xFFFFu >> (16u - hi)) & ~((1u << lo) - 1u);
            }
            my_changes += (uint32_t)__popc(d);
            while (__any(d != 0)) {  // a round: every lane that still holds a change takes its lowest
                bool has = false;
                uint64_t key = 0;
                if (d) {
                    const int j = __ffs((int)d) - 1;
                    d &= d - 1;
                    const uint32_t pos = (uint32_t)(j - first);
                    if (pos >= (uint32_t)RC_RECUR_FLANK && pos + (uint32_t)RC_RECUR_FLANK < len) {
                        uint64_t w;
                        if (rc_recur_fetch(rd + pos - RC_RECUR_FLANK, &w)) {
                            // (selected without indexing the array at run time: that would put it into scratch memory)
                            const uint32_t wo = j < 8 ? (j < 4 ? ow[0] : ow[1]) : (j < 12 ? ow[2] : ow[3]);
                            key = rc_recur_key(w, rc_recur_from((wo >> (8 * (j & 3))) & 0xffu));
                            has = true;
                        }
                    }
                }
                const uint64_t m = __ballot(has);
                if (m) {  // (uniform) one LDS atomic for the round's keys
                    const int lead_lane = __ffsll((long long)m) - 1;
                    uint32_t base = 0;
                    if ((int)lane == lead_lane) base = atomicAdd(&s_n, (uint32_t)__popcll(m));
                    base = (uint32_t)__shfl((int)base, lead_lane, 64);
                    if (has) {
                        ++my_keys;
                        const uint32_t at = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
                        if (at < RC_RECUR_STAGE)
                            s_key[at] = key;
                        else
                            over = true, over_key = key;  // (the stage is full: this one goes out on its own, below)
                    }
                }
                // a key that found the stage full: appended directly, one global atomic per wavefront and round (reads with
                // hundreds of changes; the reserved stage slot at or past RC_RECUR_STAGE is never read)
                const uint64_t mo = __ballot(over);
                if (mo) {
                    const int lead_lane = __ffsll((long long)mo) - 1;
                    unsigned long long base = 0;
                    if ((int)lane == lead_lane) base = atomicAdd(&counts[2], (unsigned long long)__popcll(mo));
                    base = ((unsigned long long)(uint32_t)__shfl((int)(uint32_t)(base >> 32), lead_lane, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)base, lead_lane, 64);
                    if (over) {
                        const unsigned long long at = base + (unsigned long long)__popcll(mo & ((1ull << lane) - 1ull));
                        if (at < cap) keys[at] = over_key;
                        over = false;
                    }
                }
            }
        }
        // the workgroup's staged keys go out once the stage is half full: one global atomic for hundreds of keys
        // (the decision must be the whole workgroup's: s_n is read between two barriers, so no wavefront that is already in the
        // next step can add to it before every wavefront has looked)
        __syncthreads();
        const uint32_t staged = s_n;
        __syncthreads();
        if (staged > RC_RECUR_STAGE / 2) flush();
    }
    __syncthreads();
    if (s_n) flush();
    if (my_changes) atomicAdd(&s_tot[0], my_changes);
    if (my_keys) atomicAdd(&s_tot[1], my_keys);
    __syncthreads();
    if (threadIdx.x < 2 && s_tot[threadIdx.x]) atomicAdd(&counts[threadIdx.x], (unsigned long long)s_tot[threadIdx.x]);
}

int rc_launch_change_keys(rc_ctx *ctx, hipStream_t st, const uint8_t *d_before, const uint8_t *d_after, const uint32_t *d_off, uint32_t n_reads, size_t nbytes,
                          uint64_t *d_keys, uint64_t cap, uint64_t *d_counts)
{
    RC_CHECK_HIP(ctx, hipMemsetAsync(d_counts, 0, 3 * sizeof(uint64_t), st));
    if (n_reads == 0 || nbytes == 0) return RC_OK;
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "change keys: arena of %zu bytes exceeds the 4 GiB batch limit", nbytes);
        return RC_ERR_ARG;
    }
    const ptrdiff_t delta = d_before - d_after;
    if (delta & 15) {
        rc_set_error(ctx, "change keys: the two arenas must have the same alignment modulo 16");
        return RC_ERR_ARG;
    }
    // persistent workgroups: eight of 256 threads fill a CU's wave slots
    unsigned g = (n_reads + RC_RECUR_QUARTERS - 1) / RC_RECUR_QUARTERS;
    if (g > (unsigned)ctx->n_cu * 8u) g = (unsigned)ctx->n_cu * 8u;
    hipLaunchKernelGGL(k_change_keys, dim3(g), dim3(RC_RECUR_THREADS), 0, st, d_after, delta, d_off, n_reads, (uint32_t)nbytes, d_keys, (unsigned long long)cap,
                       reinterpret_cast<unsigned long long *>(d_counts));
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// ---- the census of a key array ---------------------------------------------------------------------------------------------
#define RC_RECUR_LDS_BINS 1024
// every run (a site and its changes) into hist[min(length, max_bin)]; stat[0] += sites with two changes or more, stat[1] += their
// changes, stat[2] += sites with min_count changes or more; inv[i] = ~length (ascending: the longest run first)
__global__ __launch_bounds__(256) void k_recur_runs(const uint32_t *__restrict__ cnt, uint32_t n_runs, uint32_t max_bin, uint32_t min_count,
                                                    unsigned long long *__restrict__ hist, unsigned long long *__restrict__ stat, uint32_t *__restrict__ inv)
{
    __shared__ uint32_t s_bin[RC_RECUR_LDS_BINS];
    __shared__ unsigned long long s_stat[3];
    for (uint32_t b = threadIdx.x; b < RC_RECUR_LDS_BINS; b += 256u) s_bin[b] = 0;
    if (threadIdx.x < 3) s_stat[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n_runs) {
        const uint32_t run = cnt[i], bin = run < max_bin ? run : max_bin;
        inv[i] = ~run;
        if (bin < RC_RECUR_LDS_BINS)
            atomicAdd(&s_bin[bin], 1u);
        else
            atomicAdd(&hist[bin], 1ull);
        if (run >= 2u) {
            atomicAdd(&s_stat[0], 1ull);
            atomicAdd(&s_stat[1], (unsigned long long)run);
        }
        if (run >= min_count) atomicAdd(&s_stat[2], 1ull);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RC_RECUR_LDS_BINS; b += 256u) {
        const uint32_t v = s_bin[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);  // (b <= max_bin: only such bins were added to)
    }
    if (threadIdx.x < 3 && s_stat[threadIdx.x]) atomicAdd(&stat[threadIdx.x], s_stat[threadIdx.x]);
}

// d_keys: n keys, left as they are.  recur[max_bin + 1], top_key / top_count[max_sites] and the five numbers on the host.
int rc_recur_census_run(rc_ctx *ctx, const uint64_t *d_keys, size_t n, uint32_t max_bin, uint32_t min_count, uint32_t max_sites, uint64_t *recur,
                        uint64_t *sites, uint64_t *sites_recurrent, uint64_t *changes_at_recurrent, uint64_t *top_key, uint64_t *top_count, uint32_t *n_top)
{
    std::fill(recur, recur + max_bin + 1, 0ull);
    *sites = *sites_recurrent = *changes_at_recurrent = 0;
    *n_top = 0;
    if (n == 0) return RC_OK;
    if (n >= (1ull << 32)) {
        rc_set_error(ctx, "recurrence census: %zu keys are more than the census indexes (2^32 - 1)", n);
        return RC_ERR_ARG;
    }
    hipStream_t st = ctx->stream;
    size_t t_sort = 0, t_rle = 0, t_top = 0;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_keys(nullptr, t_sort, (uint64_t *)nullptr, (uint64_t *)nullptr, n, 0, 64, st));
    RC_CHECK_HIP(ctx, rocprim::run_length_encode(nullptr, t_rle, (uint64_t *)nullptr, n, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, st));
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t_top, (uint32_t *)nullptr, (uint32_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, n, 0, 32, st));
    const size_t t_bytes = std::max(std::max(t_sort, t_rle), t_top) + 256, hist_bytes = ((size_t)max_bin + 1 + 4) * 8;
    rc_dev_tmp b_a, b_b, b_cnt, b_inv, b_inv2, b_tmp, b_hist;
    if (b_a.alloc(n * 8) != hipSuccess || b_b.alloc(n * 8) != hipSuccess || b_cnt.alloc(n * 4) != hipSuccess || b_inv.alloc(n * 4) != hipSuccess ||
        b_inv2.alloc(n * 4) != hipSuccess || b_tmp.alloc(t_bytes) != hipSuccess || b_hist.alloc(hist_bytes) != hipSuccess) {
        (void)hipGetLastError();
        rc_set_error(ctx, "recurrence census: no device memory to sort %zu keys (%zu MB wanted beside the keys)", n, (n * 28 + t_bytes + hist_bytes) >> 20);
        return RC_ERR_NOMEM;
    }
    uint64_t *a = b_a.as<uint64_t>(), *b = b_b.as<uint64_t>();
    uint32_t *cnt = b_cnt.as<uint32_t>(), *inv = b_inv.as<uint32_t>(), *inv2 = b_inv2.as<uint32_t>();
    unsigned long long *hist = b_hist.as<unsigned long long>(), *stat = hist + max_bin + 1;  // (stat[3]: the number of runs, as the encode leaves it)
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_hist.p, 0, hist_bytes, st));
    size_t t = t_bytes;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_keys(b_tmp.p, t, d_keys, a, n, 0, 64, st));
    t = t_bytes;
    RC_CHECK_HIP(ctx, rocprim::run_length_encode(b_tmp.p, t, a, n, b, cnt, reinterpret_cast<uint32_t *>(stat + 3), st));  // b: the sites, ascending
    uint32_t n_runs = 0;
    RC_CHECK_HIP(ctx, hipMemcpyAsync(&n_runs, stat + 3, 4, hipMemcpyDeviceToHost, st));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(st));
    if (n_runs == 0 || n_runs > n) {
        rc_set_error(ctx, "recurrence census: internal: %u runs of %zu keys", n_runs, n);
        return RC_ERR_STATE;
    }
    hipLaunchKernelGGL(k_recur_runs, dim3((n_runs + 255u) / 256u), dim3(256), 0, st, cnt, n_runs, max_bin, min_count, hist, stat, inv);
    RC_CHECK_HIP(ctx, hipGetLastError());
    std::vector<uint64_t> h((size_t)max_bin + 1 + 3);
    RC_CHECK_HIP(ctx, hipMemcpyAsync(h.data(), hist, h.size() * 8, hipMemcpyDeviceToHost, st));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(st));
    std::copy(h.begin(), h.begin() + max_bin + 1, recur);
    recur[0] = 0;
    *sites = n_runs;
    *sites_recurrent = h[max_bin + 1];
    *changes_at_recurrent = h[max_bin + 2];
    const uint64_t qualify = h[max_bin + 3];
    const uint32_t top = (uint32_t)std::min<uint64_t>(qualify, max_sites);
    if (top) {
        t = t_bytes;
        RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(b_tmp.p, t, inv, inv2, b, a, n_runs, 0, 32, st));  // stable: equal counts keep the keys' ascending order
        std::vector<uint32_t> hc(top);
        RC_CHECK_HIP(ctx, hipMemcpyAsync(top_key, a, (size_t)top * 8, hipMemcpyDeviceToHost, st));
        RC_CHECK_HIP(ctx, hipMemcpyAsync(hc.data(), inv2, (size_t)top * 4, hipMemcpyDeviceToHost, st));
        RC_CHECK_HIP(ctx, hipStreamSynchronize(st));
        for (uint32_t i = 0; i < top; ++i) top_count[i] = (uint64_t)(uint32_t)~hc[i];
    }
    *n_top = top;
    return RC_OK;
}
