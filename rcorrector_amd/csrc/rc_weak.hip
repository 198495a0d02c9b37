// rc_weak.hip -- the per-read weak-k-mer profile (include/rcorrector_amd.h: rc_read_weak; arithmetic in rc_weak.h): which
// k-windows of every read of an arena the table holds at least min_count times, reduced to four numbers per read.
//
// Two launches.  k_weak_planes probes every k-window of the arena out of k_probe's tile (rc_device.h: rc_tile_stage; rc_common.h:
// rc_tile_window; one bucket probe per valid window) but keeps one bit per window in two planes, solid and weak, instead of a
// count: a wavefront ballots 64 consecutive positions into one
// 64-bit word per plane, owns 1 KiB of the tile and so sixteen consecutive words of each plane, and writes them as one
// 128-byte row -- 0.25 bytes per base against k_probe's 4.  k_weak_reduce then takes one read per lane: the (at most 17 for
// 1 023 bases) words of each plane the read spans, through rc_weak_reduce.
// The arena may start anywhere: rc_tile_stage reads it from the 16-byte boundary at or in front of its first byte, `lead` bytes
// in front of it, and the planes are indexed by position + lead.
#include "rc_device.h"
#include "rc_internal.h"
#include "rc_weak.h"

#define RC_WEAK_WAVE_BYTES (RC_PROBE_TILE / (RC_PROBE_THREADS / 64))  // arena bytes of a tile one wavefront owns
#define RC_WEAK_WAVE_WORDS (RC_WEAK_WAVE_BYTES / 64)                  // ... and the plane words they make
static_assert(RC_WEAK_WAVE_WORDS <= 64, "a lane keeps one plane word of its wavefront");

// seq16: the 16-byte boundary at or in front of the arena; the arena is bytes [lead, lead + nbytes) from there.
// solid / weak: RC_PROBE_TILE / 64 words per tile of the grid, every one of them written.
template <bool EXT>
__global__ __launch_bounds__(RC_PROBE_THREADS) void k_weak_planes(rc_table_view T, const uint8_t *__restrict__ seq16, uint32_t lead, size_t nbytes,
                                                                  int k, int min_count, uint64_t *__restrict__ solid, uint64_t *__restrict__ weak)
{
    __shared__ uint32_t s_code[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_inv[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_nul[RC_PROBE_TILE / 16 + 4];
    const size_t tile0 = (size_t)blockIdx.x * RC_PROBE_TILE;
    const int t = threadIdx.x;
    rc_tile_stage(seq16, lead, nbytes, tile0, s_code, s_inv, s_nul);
    __syncthreads();
    const uint32_t *m_inv = reinterpret_cast<const uint32_t *>(s_inv);
    const uint32_t *m_nul = reinterpret_cast<const uint32_t *>(s_nul);

    // wavefront wv owns bytes [wv * RC_WEAK_WAVE_BYTES, +RC_WEAK_WAVE_BYTES) of the tile, 64 consecutive positions a step: the
    // lanes of a step read one or two words of each mask (a broadcast) and five consecutive code words
    const int wv = t >> 6, ln = t & 63;
    uint64_t keep_s = 0, keep_w = 0;
#pragma unroll 2
    for (int it = 0; it < RC_WEAK_WAVE_WORDS; ++it) {
        const int a = wv * RC_WEAK_WAVE_BYTES + it * 64 + ln;
        const rc_tile_win w = rc_tile_window(s_code, m_inv, m_nul, a, k);
        // a window of k bytes, all of them ACGT, none a NUL (a read's end, or the arena's)
        const bool valid = !w.nul && !w.bad;
        const int cnt = valid ? rc_table_lookup<EXT>(T, rc_canonical(w.code, k)) : 0;
        const uint64_t bs = __ballot(valid && cnt >= min_count), bw = __ballot(valid && cnt < min_count);
        if (ln == it) {
            keep_s = bs;
            keep_w = bw;
        }
    }
    if (ln < RC_WEAK_WAVE_WORDS) {  // one 128-byte row per plane and wavefront
        const size_t w = (tile0 >> 6) + (size_t)wv * RC_WEAK_WAVE_WORDS + (size_t)ln;
        solid[w] = keep_s;
        weak[w] = keep_w;
    }
}

// one read per lane: consecutive lanes take consecutive reads, whose plane words are neighbours
__global__ __launch_bounds__(256) void k_weak_reduce(const uint64_t *__restrict__ solid, const uint64_t *__restrict__ weak, uint32_t lead,
                                                     size_t nbytes, const uint32_t *__restrict__ off, uint32_t n, int k,
                                                     rc_weak_vals *__restrict__ out)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t g0 = off[r], g1 = off[r + 1];
    // (a read is its bases and a NUL; offsets that leave the arena describe no read: the planes end with it)
    const int32_t L = g1 > g0 && (size_t)g1 <= nbytes ? (int32_t)(g1 - g0) - 1 : 0;
    out[r] = rc_weak_reduce(solid, weak, (uint64_t)g0 + lead, L, k);
}

int rc_launch_weak_planes(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, int min_count, rc_dbuf *planes, const uint64_t **solid_out,
                          const uint64_t **weak_out, uint32_t *lead_out)
{
    const uint32_t lead = (uint32_t)((uintptr_t)d_seq & 15u);
    const size_t span = (size_t)lead + nbytes;
    const unsigned G = (unsigned)((span + RC_PROBE_TILE - 1) / RC_PROBE_TILE);
    const size_t plane_words = (size_t)(G ? G : 1) * (RC_PROBE_TILE / 64);
    if (const int rc = rc_dbuf_reserve(ctx, planes, plane_words * 16)) return rc;
    uint64_t *solid = (uint64_t *)planes->p, *weak = solid + plane_words;
    if (G)
        rc_with_ext(ctx->ext, [&](auto ext) {
            hipLaunchKernelGGL(k_weak_planes<decltype(ext)::value>, dim3(G), dim3(RC_PROBE_THREADS), 0, ctx->stream, rc_view(ctx), d_seq - lead, lead, nbytes,
                               ctx->k, min_count, solid, weak);
        });
    *solid_out = solid;
    *weak_out = weak;
    *lead_out = lead;
    return RC_OK;
}

int rc_launch_weak_profile(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int min_count, rc_dbuf *planes,
                           void *d_out)
{
    if (n_reads == 0) return RC_OK;
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "weak_profile: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    static_assert(sizeof(rc_weak_vals) == 16, "rc_read_weak");
    const uint64_t *solid, *weak;
    uint32_t lead;
    rc_timer_begin(ctx);
    if (const int rc = rc_launch_weak_planes(ctx, d_seq, nbytes, min_count, planes, &solid, &weak, &lead)) return rc;
    hipLaunchKernelGGL(k_weak_reduce, dim3((n_reads + 255) / 256), dim3(256), 0, ctx->stream, solid, weak, lead, nbytes, d_off, n_reads, ctx->k,
                       (rc_weak_vals *)d_out);
    rc_timer_end(ctx, RC_T_WEAK);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
