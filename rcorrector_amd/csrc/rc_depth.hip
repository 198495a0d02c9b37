// rc_depth.hip -- the per-read k-mer depth (include/rcorrector_amd.h: rc_read_depth; arithmetic in rc_depth.h): for every read
// of an arena the number of its valid k-windows and the lower quartile, median and upper quartile of their counts in the table.
//
// One launch.  A workgroup takes RC_RUN_BLOCK_READS consecutive reads, a run of them that fits the probe tile at a time: the run
// is staged in LDS by rc_tile_stage_run (rc_device.h: where the arena may start, which read is no read -- four zeros here)
// and cut into windows as k_probe_list does it (rc_common.h: rc_tile_window), one bucket probe per valid window -- but the
// counts stay in LDS, 4 bytes per local position over the bytes the raw copy no longer needs, RC_DEPTH_INVALID for a window that
// is no k-mer.  A wavefront then takes a read: its lanes hold the read's counts, ceil(windows / 64) each, and rc_depth_select
// finds the three ranks in one descent over the counts' bits, a ballot and a population count per value slot and question.
// 16 bytes per read leave the kernel.
#include "rc_device.h"
#include "rc_internal.h"
#include "rc_depth.h"

// the depth of one read by one wavefront: cnt[0 .. nwin) in LDS, NV * 64 >= nwin
template <int NV>
__device__ __forceinline__ rc_depth_vals rc_depth_wave(const uint32_t *cnt, uint32_t nwin, uint32_t ln)
{
    uint32_t v[NV], orv = 0, n = 0;
#pragma unroll
    for (int s = 0; s < NV; ++s) {
        const uint32_t i = 64u * (uint32_t)s + ln;
        v[s] = i < nwin ? cnt[i] : RC_DEPTH_INVALID;
        const bool ok = v[s] != RC_DEPTH_INVALID;
        n += (uint32_t)__popcll(__ballot(ok));
        orv |= ok ? v[s] : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) orv |= (uint32_t)__shfl_xor((int)orv, o, 64);
    orv = (uint32_t)__builtin_amdgcn_readfirstlane((int)orv);  // (the same in every lane: the descent's loop is the wavefront's)
    return rc_depth_select(n, orv, [&](int shift, uint32_t key) {
        uint32_t c = 0;
#pragma unroll
        for (int s = 0; s < NV; ++s) c += (uint32_t)__popcll(__ballot((v[s] >> shift) == key));
        return c;
    });
}

// seq16: the 16-byte boundary at or in front of the arena; the arena is bytes [lead, lead + nbytes) from there, off counts from
// its first byte.  out[r] is written for every r < n.
template <bool EXT>
__global__ __launch_bounds__(RC_PROBE_THREADS) void k_read_depth(rc_table_view T, const uint8_t *__restrict__ seq16, uint32_t lead, size_t nbytes,
                                                                 const uint32_t *__restrict__ off, uint32_t n, int k, rc_depth_vals *__restrict__ out)
{
    // the run's bytes as copied (RC_PROBE_TILE + 64 of them), then -- the planes packed -- the counts of its local positions
    __shared__ __attribute__((aligned(16))) uint32_t s_cnt[RC_PROBE_TILE];
    __shared__ uint32_t s_code[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_inv[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_nul[RC_PROBE_TILE / 16 + 4];
    __shared__ uint32_t s_lpos[RC_RUN_BLOCK_READS + 1], s_gpos[RC_RUN_BLOCK_READS], s_len1[RC_RUN_BLOCK_READS];
    __shared__ uint32_t s_take;
    uint32_t *s_raw = s_cnt;
    const uint32_t t = threadIdx.x, wv = t >> 6, ln = t & 63u;
    const uint32_t i0 = blockIdx.x * (uint32_t)RC_RUN_BLOCK_READS;
    const uint32_t nr_all = n - i0 < (uint32_t)RC_RUN_BLOCK_READS ? n - i0 : (uint32_t)RC_RUN_BLOCK_READS;
    const uint32_t *m_inv = reinterpret_cast<const uint32_t *>(s_inv);
    const uint32_t *m_nul = reinterpret_cast<const uint32_t *>(s_nul);
    for (uint32_t done = 0; done < nr_all;) {
        uint32_t total;  // (the local end of the run's last read)
        const uint32_t nr = rc_tile_stage_run<RC_PROBE_THREADS>(s_raw, s_code, s_inv, s_nul, s_lpos, s_gpos, s_len1, &s_take, seq16, lead, nbytes, off,
                                                                i0 + done, nr_all - done, &total);
        // (from here on s_raw's words are s_cnt's)
#pragma unroll 2
        for (uint32_t a = 4u + t; a + (uint32_t)k <= total; a += RC_PROBE_THREADS) {
            const rc_tile_win w = rc_tile_window(s_code, m_inv, m_nul, (int)a, k);
            s_cnt[a] = w.nul || w.bad ? RC_DEPTH_INVALID : (uint32_t)rc_table_lookup<EXT>(T, rc_canonical(w.code, k));
        }
        __syncthreads();
        for (uint32_t j = wv; j < nr; j += RC_PROBE_THREADS / 64) {  // a wavefront per read
            const uint32_t len1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_len1[j]);
            const uint32_t nwin = len1 > (uint32_t)k ? len1 - (uint32_t)k : 0u;  // L - k + 1 with L = len1 - 1
            const uint32_t *cnt = s_cnt + s_lpos[j];
            rc_depth_vals d = {0, 0, 0, 0};
            if (nwin > 256u)
                d = rc_depth_wave<RC_MAX_READ_LENGTH / 64>(cnt, nwin, ln);
            else if (nwin > 128u)
                d = rc_depth_wave<4>(cnt, nwin, ln);
            else if (nwin)
                d = rc_depth_wave<2>(cnt, nwin, ln);
            if (ln == 0) out[i0 + done + j] = d;
        }
        done += nr;
        __syncthreads();  // (the next run rewrites the tile)
    }
}

int rc_launch_read_depth(rc_ctx *ctx, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, void *d_out)
{
    if (n_reads == 0) return RC_OK;
    if (!ctx->d_buckets) {
        rc_set_error(ctx, "read_depth: no k-mer table loaded");
        return RC_ERR_STATE;
    }
    static_assert(sizeof(rc_depth_vals) == 16, "rc_read_depth");
    const uint32_t lead = (uint32_t)((uintptr_t)d_seq & 15u);
    if ((uint64_t)nbytes >= (1ull << 32)) {  // (wherever it starts: rc_tile_stage_run's positions from the boundary in front of it may pass 2^32)
        rc_set_error(ctx, "read_depth: arena of %zu bytes exceeds the 4 GiB batch limit", nbytes);
        return RC_ERR_ARG;
    }
    const unsigned G = (unsigned)(((uint64_t)n_reads + RC_RUN_BLOCK_READS - 1) / RC_RUN_BLOCK_READS);
    rc_timer_begin(ctx);
    rc_with_ext(ctx->ext, [&](auto ext) {
        hipLaunchKernelGGL(k_read_depth<decltype(ext)::value>, dim3(G), dim3(RC_PROBE_THREADS), 0, ctx->stream, rc_view(ctx), d_seq - lead, lead, nbytes, d_off,
                           n_reads, ctx->k, (rc_depth_vals *)d_out);
    });
    rc_timer_end(ctx, RC_T_DEPTH);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
