// rc_screen.hip -- the per-read hit profile against a second k-mer set (include/rcorrector_amd.h: rc_read_screen; arithmetic in
// rc_screen.h): for every read of an arena its valid k-windows, those whose canonical k-mer a SCREEN table -- any context's, not
// the one the kernel runs in -- holds at least min_count times, the bases such windows cover and their longest run.
//
// One launch.  A workgroup takes RC_RUN_BLOCK_READS consecutive reads, a run of them that fits the probe tile at a time, staged
// in LDS by rc_tile_stage_run (rc_device.h: where the arena may start, which read is no read -- four zeros here), as
// k_read_depth (rc_depth.hip) does.  What follows differs: nothing but a bit per window has to survive the probe, so no count
// is kept anywhere.  A wavefront takes a read, 64 windows at a time, one bucket probe per valid window into the screen table,
// and the two ballots -- valid, hit -- are the next word of the read's masks, uniform in the wavefront: the valid one is
// counted, the hit one goes through rc_screen_add_word, the same run-by-run walk the host program checks.  16 bytes per read
// leave the kernel.
#include "rc_device.h"
#include "rc_internal.h"
#include "rc_screen.h"

// S: the screen table.  seq16: the 16-byte boundary at or in front of the arena; the arena is bytes [lead, lead + nbytes) from
// there, off counts from its first byte.  out[r] is written for every r < n.
template <bool EXT>
__global__ __launch_bounds__(RC_PROBE_THREADS) void k_read_screen(rc_table_view S, const uint8_t *__restrict__ seq16, uint32_t lead, size_t nbytes,
                                                                  const uint32_t *__restrict__ off, uint32_t n, int k, int min_count,
                                                                  rc_screen_vals *__restrict__ out)
{
    __shared__ __attribute__((aligned(16))) uint32_t s_raw[(RC_PROBE_TILE + 64) / 4];  // the run's bytes as copied
    __shared__ uint32_t s_code[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_inv[RC_PROBE_TILE / 16 + 4];
    __shared__ uint16_t s_nul[RC_PROBE_TILE / 16 + 4];
    __shared__ uint32_t s_lpos[RC_RUN_BLOCK_READS + 1], s_gpos[RC_RUN_BLOCK_READS], s_len1[RC_RUN_BLOCK_READS];
    __shared__ uint32_t s_take;
    const uint32_t t = threadIdx.x, wv = t >> 6, ln = t & 63u;
    const uint32_t i0 = blockIdx.x * (uint32_t)RC_RUN_BLOCK_READS;
    const uint32_t nr_all = n - i0 < (uint32_t)RC_RUN_BLOCK_READS ? n - i0 : (uint32_t)RC_RUN_BLOCK_READS;
    const uint32_t *m_inv = reinterpret_cast<const uint32_t *>(s_inv);
    const uint32_t *m_nul = reinterpret_cast<const uint32_t *>(s_nul);
    for (uint32_t done = 0; done < nr_all;) {
        const uint32_t nr = rc_tile_stage_run<RC_PROBE_THREADS>(s_raw, s_code, s_inv, s_nul, s_lpos, s_gpos, s_len1, &s_take, seq16, lead, nbytes, off,
                                                                i0 + done, nr_all - done);
        for (uint32_t j = wv; j < nr; j += RC_PROBE_THREADS / 64) {  // a wavefront per read
            const uint32_t len1 = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_len1[j]);
            const uint32_t lp = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_lpos[j]);
            const uint32_t nwin = len1 > (uint32_t)k ? len1 - (uint32_t)k : 0u;  // L - k + 1 with L = len1 - 1
            rc_screen_acc acc;
            uint32_t valid = 0;
            for (uint32_t w0 = 0; w0 < nwin; w0 += 64u) {  // (window w0 + ln < nwin lies inside the read: lp + nwin + k = the read's NUL + 1)
                bool ok = false, hit = false;
                if (w0 + ln < nwin) {
                    const rc_tile_win w = rc_tile_window(s_code, m_inv, m_nul, (int)(lp + w0 + ln), k);
                    ok = !w.bad;  // (a NUL inside the read is a letter outside ACGT like any other)
                    if (ok) hit = rc_table_lookup<EXT>(S, rc_canonical(w.code, k)) >= min_count;
                }
                valid += (uint32_t)__popcll(__ballot(ok));
                rc_screen_add_word(acc, (uint64_t)__ballot(hit), nwin - w0 < 64u ? nwin - w0 : 64u, k);
            }
            if (ln == 0) out[i0 + done + j] = rc_screen_finish(acc, valid, k);
        }
        done += nr;
        __syncthreads();  // (the next run rewrites the tile)
    }
}

int rc_launch_read_screen(rc_ctx *ctx, const rc_ctx *screen, const uint8_t *d_seq, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int min_count,
                          void *d_out)
{
    if (n_reads == 0) return RC_OK;
    if (!screen->d_buckets) {
        rc_set_error(ctx, "read_screen: no k-mer table in the screen context");
        return RC_ERR_STATE;
    }
    if (screen->k != ctx->k || screen->device != ctx->device) {  // (the view's arithmetic is k's, its pointer the device's)
        rc_set_error(ctx, "read_screen: the screen table is of k = %d on device %d, the context of k = %d on device %d", screen->k, screen->device, ctx->k,
                     ctx->device);
        return RC_ERR_ARG;
    }
    static_assert(sizeof(rc_screen_vals) == 16, "rc_read_screen");
    const uint32_t lead = (uint32_t)((uintptr_t)d_seq & 15u);
    if ((uint64_t)nbytes >= (1ull << 32)) {  // (wherever it starts: rc_tile_stage_run's positions from the boundary in front of it may pass 2^32)
        rc_set_error(ctx, "read_screen: arena of %zu bytes exceeds the 4 GiB batch limit", nbytes);
        return RC_ERR_ARG;
    }
    const unsigned G = (unsigned)(((uint64_t)n_reads + RC_RUN_BLOCK_READS - 1) / RC_RUN_BLOCK_READS);
    rc_timer_begin(ctx);
    rc_with_ext(screen->ext, [&](auto ext) {  // (the screen table's layout, not the context's)
        hipLaunchKernelGGL(k_read_screen<decltype(ext)::value>, dim3(G), dim3(RC_PROBE_THREADS), 0, ctx->stream, rc_view(screen), d_seq - lead, lead, nbytes,
                           d_off, n_reads, ctx->k, min_count, (rc_screen_vals *)d_out);
    });
    rc_timer_end(ctx, RC_T_SCREEN);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
