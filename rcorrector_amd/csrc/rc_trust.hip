// rc_trust.hip -- the k-mer trust profile by read position (include/rcorrector_amd.h: rc_trust_profile; arithmetic in
// rc_trust.h): how many reads have a SOLID / a WEAK k-window at position p from the 5' end and from the 3' end, per mate.
//
// Three launches.  k_weak_planes (rc_weak.hip, as the per-read weak profile launches it) turns the arena into the two bit
// planes.  k_trust_accumulate reduces them across reads: a wavefront takes a contiguous run of the reads of ONE mate (the
// mate is blockIdx.y), and for word j of a read's window string lane l owns position 64 j + l -- the word is the same in
// every lane (the plane words are fetched through wave-uniform addresses), a lane adds its bit to its own 32-bit counter.
// The 5' words are rc_weak_word's, the 3' words the same string taken right-aligned and reversed (rc_trust_word3), so lane l
// owns p3 = 64 j + l there.  5 NW counters a lane (windows, solid5, weak5, solid3, weak3) in registers: the j loops have
// compile-time bounds, NW = 4 for reads of up to 256 windows and NW = 16 for everything a profile holds.  No atomics: a
// wavefront writes its counters once, as 5 NW rows of 64 consecutive uint32 into a partials buffer, and k_trust_reduce sums
// the columns into the caller's uint64 counts (which it adds to) -- the same sums in the same order on every run.
#include <algorithm>

#include "rc_device.h"
#include "rc_internal.h"
#include "rc_trust.h"

#define RC_TRUST_THREADS 256
#define RC_TRUST_WAVES (RC_TRUST_THREADS / 64)
#define RC_TRUST_ARRAYS 5  // rc_trust_counts: windows, solid5, weak5, solid3, weak3
static_assert(RC_TRUST_LEN == 16 * 64, "the wide instance holds every position of a profile");

// part: one row of RC_TRUST_ARRAYS * NW * 64 uint32 per wavefront, rows of mate 0 first: row = mate * waves + wave, entry
// (array * NW + j) * 64 + lane.  Every row is written, by wavefronts without reads too.
template <int NW>
__global__ __launch_bounds__(RC_TRUST_THREADS) void k_trust_accumulate(const uint64_t *__restrict__ solid, const uint64_t *__restrict__ weak, uint32_t lead,
                                                                       size_t nbytes, const uint32_t *__restrict__ off, uint32_t n, int mode, int k,
                                                                       uint32_t *__restrict__ part)
{
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const uint32_t waves = gridDim.x * RC_TRUST_WAVES, w = blockIdx.x * RC_TRUST_WAVES + wv, mate = blockIdx.y;
    // the reads of this mate, numbered 0 .. nm - 1: read first + step * i
    // (mode 2 with an odd number of reads: the last one is an even read, mate 0)
    const uint32_t nm = mode == 0 ? n : mode == 1 ? n >> 1 : (n + 1u - mate) >> 1;
    const uint32_t first = mode == 1 ? mate * nm : mate, step = mode == 2 ? 2u : 1u;
    const uint32_t per = (uint32_t)(((uint64_t)nm + waves - 1) / waves);
    const uint64_t lo64 = (uint64_t)w * per;
    const uint32_t lo = lo64 < nm ? (uint32_t)lo64 : nm, hi = nm - lo < per ? nm : lo + per;

    uint32_t c_win[NW], c_s5[NW], c_w5[NW], c_s3[NW], c_w3[NW];
#pragma unroll
    for (int j = 0; j < NW; ++j) c_win[j] = c_s5[j] = c_w5[j] = c_s3[j] = c_w3[j] = 0;

    for (uint32_t i = lo; i < hi; ++i) {
        const uint32_t r = first + step * i;
        const uint32_t g0 = off[r], g1 = off[r + 1];
        // (a read is its bases and a NUL; offsets that leave the arena describe no read: the planes end with it)
        const int32_t L = g1 > g0 && (size_t)g1 <= nbytes ? (int32_t)(g1 - g0) - 1 : 0;
        uint32_t nwin = rc_trust_nwin(L, k);
        if (nwin > 64u * NW) nwin = 64u * NW;  // (a read longer than the batch was said to hold: never outside the counters)
        const uint64_t bit0 = (uint64_t)g0 + lead;
#pragma unroll
        for (int j = 0; j < NW; ++j) {
            if (nwin > 64u * j) {  // (the same in every lane)
                c_win[j] += (uint32_t)(rc_trust_have(j, nwin) >> ln) & 1u;
                c_s5[j] += (uint32_t)(rc_weak_word(solid, bit0, j, nwin) >> ln) & 1u;
                c_w5[j] += (uint32_t)(rc_weak_word(weak, bit0, j, nwin) >> ln) & 1u;
                c_s3[j] += (uint32_t)(rc_trust_word3(solid, bit0, j, nwin) >> ln) & 1u;
                c_w3[j] += (uint32_t)(rc_trust_word3(weak, bit0, j, nwin) >> ln) & 1u;
            }
        }
    }

    uint32_t *row = part + ((size_t)mate * waves + w) * (RC_TRUST_ARRAYS * NW * 64) + ln;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
        row[(0 * NW + j) * 64] = c_win[j];
        row[(1 * NW + j) * 64] = c_s5[j];
        row[(2 * NW + j) * 64] = c_w5[j];
        row[(3 * NW + j) * 64] = c_s3[j];
        row[(4 * NW + j) * 64] = c_w3[j];
    }
}

// one workgroup per 64 columns of the partials (array a, mate m, word j): 16 wavefronts take every 16th row, their sums meet
// in LDS in a fixed order, and counts[a][m][64 j + lane] -- an rc_trust_counts, five arrays of [2][RC_TRUST_LEN] -- grows by it
__global__ __launch_bounds__(1024) void k_trust_reduce(const uint32_t *__restrict__ part, uint32_t waves, int nw, unsigned long long *__restrict__ counts)
{
    __shared__ unsigned long long s_sum[16][64];
    const uint32_t ln = threadIdx.x & 63u, sl = threadIdx.x >> 6;
    const uint32_t j = blockIdx.x % (uint32_t)nw, a = blockIdx.x / (uint32_t)nw, m = blockIdx.y;
    const size_t row_words = (size_t)RC_TRUST_ARRAYS * nw * 64;
    const uint32_t *col = part + (size_t)m * waves * row_words + ((size_t)a * nw + j) * 64 + ln;
    unsigned long long sum = 0;
    for (uint32_t w = sl; w < waves; w += 16) sum += col[(size_t)w * row_words];
    s_sum[sl][ln] = sum;
    __syncthreads();
    if (sl == 0) {
        sum = 0;
#pragma unroll
        for (int s = 0; s < 16; ++s) sum += s_sum[s][ln];
        counts[((size_t)a * 2 + m) * RC_TRUST_LEN + 64u * j + ln] += sum;
    }
}

// dst[i] += src[i], n 64-bit counts (a batch's staged counts into the profile)
__global__ __launch_bounds__(256) void k_trust_add(const unsigned long long *__restrict__ src, unsigned long long *__restrict__ dst, uint32_t n)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

int rc_launch_trust_add(rc_ctx *ctx, const void *d_src, void *d_dst, uint32_t n_words)
{
    hipLaunchKernelGGL(k_trust_add, dim3((n_words + 255) / 256), dim3(256), 0, ctx->stream, (const unsigned long long *)d_src, (unsigned long long *)d_dst,
                       n_words);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

int rc_launch_trust_profile(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int max_read_len, int mode,
                            int min_count, rc_dbuf *planes, rc_dbuf *partials, void *d_counts)
{
    if (n_reads == 0) return RC_OK;
    const uint64_t *solid, *weak;
    uint32_t lead;
    rc_timer_begin(ctx);
    if (const int rc = rc_launch_weak_planes(ctx, d_seq, nbytes, min_count, planes, &solid, &weak, &lead)) return rc;
    rc_timer_end(ctx, RC_T_TRUST_PLANES);
    // the instance: four words a read where no read of the batch has more than 256 windows.  The grid: the mates side by
    // side, together a few wavefronts per SIMD of every CU whatever the batch holds -- as many as the instance's registers
    // let a SIMD keep (NW = 4: 8; NW = 16: 4) would only lengthen the partials
    const int max_win = max_read_len >= ctx->k ? max_read_len - ctx->k + 1 : 0;
    const int nw = max_win <= 256 ? 4 : 16;
    const unsigned mates = mode == 0 ? 1u : 2u;
    const unsigned per_simd = nw == 4 ? 4u : 2u;
    const unsigned gx = std::max(1u, (unsigned)ctx->n_cu * per_simd / mates), waves = gx * RC_TRUST_WAVES;
    const size_t row_bytes = (size_t)RC_TRUST_ARRAYS * nw * 64 * 4;
    if (const int rc = rc_dbuf_reserve(ctx, partials, (size_t)mates * waves * row_bytes)) return rc;
    uint32_t *part = (uint32_t *)partials->p;
    rc_timer_begin(ctx);
    if (nw == 4)
        hipLaunchKernelGGL(k_trust_accumulate<4>, dim3(gx, mates), dim3(RC_TRUST_THREADS), 0, ctx->stream, solid, weak, lead, nbytes, d_off, n_reads, mode,
                           ctx->k, part);
    else
        hipLaunchKernelGGL(k_trust_accumulate<16>, dim3(gx, mates), dim3(RC_TRUST_THREADS), 0, ctx->stream, solid, weak, lead, nbytes, d_off, n_reads, mode,
                           ctx->k, part);
    hipLaunchKernelGGL(k_trust_reduce, dim3(RC_TRUST_ARRAYS * nw, mates), dim3(1024), 0, ctx->stream, part, waves, nw, (unsigned long long *)d_counts);
    rc_timer_end(ctx, RC_T_TRUST);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
