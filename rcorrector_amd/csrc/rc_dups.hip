// rc_dups.hip -- the duplicate census (include/rcorrector_amd.h: rc_dup_census; the keys' arithmetic in rc_dups.h): one 128-bit
// key per unit of an arena, and the census of a key array -- how many distinct keys, and how many of them occur c times.
//
// k_read_keys: a quarter wave (16 lanes) per unit, four units per wavefront (the house shape, rc_quarter.h / rc_report.hip).
// Lane l of the quarter takes chunks l, l + 16, ... of a read -- bytes [16 c, 16 c + 16) of the READ, wherever it starts: the
// arena is read in ALIGNED 16-byte pieces from the 16-byte boundary at or in front of the read, the two pieces a chunk
// straddles are shifted together (the bytes in front of the read leave with the shift), and the bytes behind the read's last
// are cleared, so nothing outside a read enters its key and the arena may start at any address.  A read of up to 256 bytes is
// one step; longer ones loop.  The lanes' sums of chunk terms meet in a row reduction (DPP: quad_perm, row_half_mirror,
// row_mirror -- no LDS), lane 0 finishes the read's key, and for a pair the quarter does mate 1, then mate 2, and combines.
// A piece that holds a byte of the arena lies in that byte's page: the loads up to 15 bytes outside it cannot fault.
//
// The census: the keys split into their two words, two stable 64-bit radix passes (low word, then high word), a head flag
// where a key differs from the one before it, a running maximum that carries every run's first index to its last element, and
// there the run's length goes into the histogram (LDS for the small bins, where nearly all runs are).
#include <algorithm>
#include <cstring>
#include <vector>
#include <rocprim/rocprim.hpp>

#include "rc_internal.h"
#include "rc_device.h"
#include "rc_dups.h"

#define RC_DUP_THREADS 256
#define RC_DUP_QUARTERS (RC_DUP_THREADS / 16)

__device__ __forceinline__ uint64_t rc_dup_row_sum(uint64_t v)
{
    // after the four steps every lane of the row holds the sum of its sixteen
#define RC_DUP_STEP(CTRL)                                                                           \
    v += ((uint64_t)rc_dpp_u32<CTRL>((uint32_t)(v >> 32)) << 32) | rc_dpp_u32<CTRL>((uint32_t)v);
    RC_DUP_STEP(0xB1)   // quad_perm [1,0,3,2]
    RC_DUP_STEP(0x4E)   // quad_perm [2,3,0,1]
    RC_DUP_STEP(0x141)  // row_half_mirror
    RC_DUP_STEP(0x140)  // row_mirror
#undef RC_DUP_STEP
    return v;
}

// the key of read r (both lanes) in every lane of the quarter that keys it; a quarter that is not live keys an empty read
__device__ __forceinline__ void rc_dup_quarter_key(const uint8_t *__restrict__ seq, uint32_t nbytes, const uint32_t *__restrict__ off, uint32_t r, bool live,
                                                   uint32_t l16, uint64_t &k0, uint64_t &k1)
{
    uint32_t o = 0, len = 0;
    if (live) {
        o = off[r];
        const uint32_t o1 = off[r + 1];
        // (offsets ascend and end inside the arena by contract; ones that do not must still not send a load outside it)
        if (o > nbytes) o = nbytes;
        const uint32_t e = o1 > nbytes ? nbytes : o1;
        len = e > o ? e - o - 1u : 0u;
    }
    const uintptr_t s = (uintptr_t)(seq + o), a0 = s & ~(uintptr_t)15;
    const uint32_t lead = (uint32_t)(s - a0);
    const uint32_t n_ch = (len + 15u) >> 4, n_pc = (lead + len + 15u) >> 4;  // chunks of the read, aligned pieces that hold them
    uint64_t sum0 = 0, sum1 = 0;
    for (uint32_t c = l16; c < n_ch; c += 16u) {
        const uint4 *pc = reinterpret_cast<const uint4 *>(a0) + c;
        const uint4 p0 = pc[0];  // (16 c < len: holds a byte of the read)
        uint4 p1 = make_uint4(0, 0, 0, 0);
        if (lead && c + 1u < n_pc) p1 = pc[1];  // (holds one too)
        // the chunk: bytes [lead, lead + 16) of the two pieces side by side (a 128-bit shift; no array for the compiler to index)
        typedef unsigned __int128 u128;
        const u128 lo = ((u128)(((uint64_t)p0.w << 32) | p0.z) << 64) | (((uint64_t)p0.y << 32) | p0.x);
        const u128 hi = ((u128)(((uint64_t)p1.w << 32) | p1.z) << 64) | (((uint64_t)p1.y << 32) | p1.x);
        const u128 ch = lead ? (lo >> (8u * lead)) | (hi << (128u - 8u * lead)) : lo;
        uint64_t a = (uint64_t)ch, b = (uint64_t)(ch >> 64);
        rc_dup_tail_mask(len - 16u * c, a, b);
        sum0 += rc_dup_chunk(a, b, c, 0);
        sum1 += rc_dup_chunk(a, b, c, 1);
    }
    k0 = rc_dup_read(rc_dup_row_sum(sum0), len, 0);
    k1 = rc_dup_read(rc_dup_row_sum(sum1), len, 1);
}

// seq: the arena, nbytes of it; off[n_reads + 1]; keys[2 * units].  mode as rc_device_batch.
__global__ __launch_bounds__(RC_DUP_THREADS) void k_read_keys(const uint8_t *__restrict__ seq, uint32_t nbytes, const uint32_t *__restrict__ off,
                                                              uint32_t n_reads, int mode, uint32_t units, uint64_t *__restrict__ keys)
{
    const uint32_t l16 = threadIdx.x & 15u;
    const uint32_t u = blockIdx.x * RC_DUP_QUARTERS + (threadIdx.x >> 4);
    const bool live = u < units;  // (no lane leaves: the row reduction wants whole rows)
    uint64_t k0, k1;
    rc_dup_quarter_key(seq, nbytes, off, mode == 2 ? 2u * u : u, live, l16, k0, k1);
    if (mode != 0) {  // (the same for every lane) the mate: the read half an arena on, or the next one
        uint64_t m0, m1;
        rc_dup_quarter_key(seq, nbytes, off, mode == 1 ? u + (n_reads >> 1) : 2u * u + 1u, live, l16, m0, m1);
        k0 = rc_dup_pair(k0, m0, 0);
        k1 = rc_dup_pair(k1, m1, 1);
    }
    if (live && l16 == 0) *reinterpret_cast<ulonglong2 *>(keys + 2 * (size_t)u) = make_ulonglong2(k0, k1);
}

int rc_launch_read_keys(rc_ctx *ctx, hipStream_t st, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int mode,
                        uint64_t *d_keys)
{
    const uint32_t units = mode == 0 ? n_reads : n_reads >> 1;
    if (units == 0) return RC_OK;
    if (nbytes >= (1ull << 32)) {
        rc_set_error(ctx, "read keys: arena of %zu bytes exceeds the 4 GiB batch limit", nbytes);
        return RC_ERR_ARG;
    }
    const unsigned g = (units + RC_DUP_QUARTERS - 1) / RC_DUP_QUARTERS;
    hipLaunchKernelGGL(k_read_keys, dim3(g), dim3(RC_DUP_THREADS), 0, st, d_seq, (uint32_t)nbytes, d_off, n_reads, mode, units, d_keys);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

// ---- the census of a key array ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_dup_split(const uint64_t *__restrict__ keys, uint32_t n, uint64_t *__restrict__ lo, uint64_t *__restrict__ hi)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const ulonglong2 k = *reinterpret_cast<const ulonglong2 *>(keys + 2 * (size_t)i);
    lo[i] = k.x;
    hi[i] = k.y;
}

// start[i] = i where the sorted key i opens a run, else 0 (the running maximum then holds every element's run start)
__global__ __launch_bounds__(256) void k_dup_heads(const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, uint32_t n, uint32_t *__restrict__ start)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    start[i] = (i > 0 && (lo[i] != lo[i - 1] || hi[i] != hi[i - 1])) ? i : 0u;
}

#define RC_DUP_LDS_BINS 1024
// the last element of every run adds the run to hist[min(length, max_bin)]
__global__ __launch_bounds__(256) void k_dup_runs(const uint64_t *__restrict__ lo, const uint64_t *__restrict__ hi, const uint32_t *__restrict__ start,
                                                  uint32_t n, uint32_t max_bin, unsigned long long *__restrict__ hist)
{
    __shared__ uint32_t s_bin[RC_DUP_LDS_BINS];
    for (uint32_t b = threadIdx.x; b < RC_DUP_LDS_BINS; b += 256u) s_bin[b] = 0;
    __syncthreads();
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n && (i + 1u == n || lo[i] != lo[i + 1] || hi[i] != hi[i + 1])) {
        const uint32_t run = i - start[i] + 1u, bin = run < max_bin ? run : max_bin;
        if (bin < RC_DUP_LDS_BINS)
            atomicAdd(&s_bin[bin], 1u);
        else
            atomicAdd(&hist[bin], 1ull);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RC_DUP_LDS_BINS; b += 256u) {
        const uint32_t v = s_bin[b];
        if (v) atomicAdd(&hist[b], (unsigned long long)v);  // (b <= max_bin: only such bins were added to)
    }
}

// d_keys: n keys of two words each, left as they are.  copies[max_bin + 1] and *distinct on the host.
int rc_dup_census_run(rc_ctx *ctx, const uint64_t *d_keys, size_t n, uint32_t max_bin, uint64_t *copies, uint64_t *distinct)
{
    std::fill(copies, copies + max_bin + 1, 0ull);
    *distinct = 0;
    if (n == 0) return RC_OK;
    if (n >= (1ull << 32)) {
        rc_set_error(ctx, "dup census: %zu units are more than the census indexes (2^32 - 1)", n);
        return RC_ERR_ARG;
    }
    hipStream_t st = ctx->stream;
    size_t t_sort = 0, t_scan = 0;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(nullptr, t_sort, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nullptr, n, 0, 64, st));
    RC_CHECK_HIP(ctx, rocprim::inclusive_scan(nullptr, t_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, n, rocprim::maximum<uint32_t>(), st));
    const size_t t_bytes = std::max(t_sort, t_scan) + 256, hist_bytes = ((size_t)max_bin + 1) * 8;
    rc_dev_tmp b_lo, b_hi, b_lo2, b_hi2, b_tmp, b_hist;
    // (the run starts live in the first pass's output of the low words, free again after the second pass)
    if (b_lo.alloc(n * 8) != hipSuccess || b_hi.alloc(n * 8) != hipSuccess || b_lo2.alloc(n * 8) != hipSuccess || b_hi2.alloc(n * 8) != hipSuccess ||
        b_tmp.alloc(t_bytes) != hipSuccess || b_hist.alloc(hist_bytes) != hipSuccess) {
        (void)hipGetLastError();
        rc_set_error(ctx, "dup census: no device memory to sort %zu keys (%zu MB wanted beside the keys)", n, (n * 32 + t_bytes + hist_bytes) >> 20);
        return RC_ERR_NOMEM;
    }
    uint64_t *lo = b_lo.as<uint64_t>(), *hi = b_hi.as<uint64_t>(), *lo2 = b_lo2.as<uint64_t>(), *hi2 = b_hi2.as<uint64_t>();
    const unsigned g = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_dup_split, dim3(g), dim3(256), 0, st, d_keys, (uint32_t)n, lo, hi);
    RC_CHECK_HIP(ctx, hipGetLastError());
    size_t t = t_bytes;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(b_tmp.p, t, lo, lo2, hi, hi2, n, 0, 64, st));  // by the low word ...
    t = t_bytes;
    RC_CHECK_HIP(ctx, rocprim::radix_sort_pairs(b_tmp.p, t, hi2, hi, lo2, lo, n, 0, 64, st));  // ... then, stable, by the high word
    uint32_t *start = reinterpret_cast<uint32_t *>(lo2), *start_s = reinterpret_cast<uint32_t *>(hi2);
    hipLaunchKernelGGL(k_dup_heads, dim3(g), dim3(256), 0, st, lo, hi, (uint32_t)n, start);
    RC_CHECK_HIP(ctx, hipGetLastError());
    t = t_bytes;
    RC_CHECK_HIP(ctx, rocprim::inclusive_scan(b_tmp.p, t, start, start_s, n, rocprim::maximum<uint32_t>(), st));
    RC_CHECK_HIP(ctx, hipMemsetAsync(b_hist.p, 0, hist_bytes, st));
    hipLaunchKernelGGL(k_dup_runs, dim3(g), dim3(256), 0, st, lo, hi, start_s, (uint32_t)n, max_bin, b_hist.as<unsigned long long>());
    RC_CHECK_HIP(ctx, hipGetLastError());
    RC_CHECK_HIP(ctx, hipMemcpyAsync(copies, b_hist.p, hist_bytes, hipMemcpyDeviceToHost, st));
    RC_CHECK_HIP(ctx, hipStreamSynchronize(st));
    copies[0] = 0;
    for (uint32_t c = 1; c <= max_bin; ++c) *distinct += copies[c];
    return RC_OK;
}
