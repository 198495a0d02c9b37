// rc_merge.hip -- merging overlapping mates into a new, compact arena on the device (include/rcorrector_amd.h:
// rc_read_merge_device; the contract in rc_merge.h).  Three steps on the context's stream:
//   * k_merge_plan: a wavefront per pair, persistent workgroups, shaped as k_read_trim's pair section (rc_trim.hip): the mates
//     staged with aligned 16-byte loads into rc_overlap.h strings in LDS, mate 2 reversed and complemented word by word, every
//     lane one offset d, 64 a round, the largest rc_ov_key by a butterfly of shuffles (rc_merge_scan_pair, the scan as a device
//     function of its own).  It leaves the unit's row and out_len[u] = merged_len + 1: an unmerged unit becomes an empty string;
//   * an exclusive scan of out_len (units + 1 entries, the last one 0) into d_moff, whose last entry is then the arena's size;
//   * k_merge_write: a wavefront per unit again.  Both mates' bases and quality bytes are staged as BYTES in LDS, 16 a lane
//     (rc_ov_load16).  The unit's F + 1 output bytes lie at [d_moff[u], d_moff[u + 1]); a lane makes one aligned 16-byte granule
//     of the output arena a round (rc_merge_granule) -- at most 129 granules, so up to three rounds, two at F > 1024 unless the
//     span starts late in its first granule.  A granule that lies inside the span goes out as one 16-byte store; the granule at
//     either end is shared with the neighbouring units, which other wavefronts write: its bytes go out one by one, and nothing is
//     ever read from the output.  Every index into an arena is a size_t.
// The counts: the plan's are wave-uniform and kept in registers, the length histogram in LDS, 32 bits a bin; k_merge_write counts
// its disagreements per lane.  Every workgroup adds its non-zero bins to the caller's 64-bit tally once, at the end.  Two
// instances of each kernel by the longest read: 8 words a mate (up to 256 bases) and 32 (up to RC_MERGE_MAX_LEN); a mate longer
// than its instance holds is cut to that in BOTH kernels, so a wrong max_read_len never indexes outside LDS.
#include <algorithm>
#include <cstddef>
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "../../include/rcorrector_amd.h"
#include "rc_internal.h"
#include "rc_merge.h"
#include "rc_overlap_stage.h"

#define RC_MERGE_THREADS 256
#define RC_MERGE_WAVES (RC_MERGE_THREADS / 64)
// the 64-bit words of an rc_merge_tally: nine totals, then len_hist
enum {
    RC_MT_PAIRS = 0, RC_MT_MERGED = 1, RC_MT_UNMERGED = 2, RC_MT_THROUGH = 3, RC_MT_COMPARED = 4, RC_MT_MISMATCH = 5, RC_MT_TOOK = 6,
    RC_MT_TOTALS = 9,
    RC_MT_BINS = RC_MT_TOTALS + RC_MERGE_LEN_BINS
};
static_assert(sizeof(rc_merge_tally) == RC_MT_BINS * 8, "the bins are an rc_merge_tally");
static_assert(offsetof(rc_merge_tally, merged) == RC_MT_MERGED * 8 && offsetof(rc_merge_tally, unmerged) == RC_MT_UNMERGED * 8 &&
                  offsetof(rc_merge_tally, readthrough) == RC_MT_THROUGH * 8 && offsetof(rc_merge_tally, compared) == RC_MT_COMPARED * 8 &&
                  offsetof(rc_merge_tally, mismatches) == RC_MT_MISMATCH * 8 && offsetof(rc_merge_tally, took_mate1) == RC_MT_TOOK * 8 &&
                  offsetof(rc_merge_tally, ties) == (RC_MT_TOOK + 2) * 8 && offsetof(rc_merge_tally, len_hist) == RC_MT_TOTALS * 8,
              "as the kernels index them");
static_assert(sizeof(rc_read_merge) == 16, "16 bytes per unit");
static_assert(RC_MERGE_MAX_OUT < RC_MERGE_LEN_BINS, "a bin for every merged length");

struct rc_merge_args {
    const uint8_t *seq, *qual;  // qual may be null
    uint32_t nbytes;
    const uint32_t *off;
    uint32_t units;
    int mode;
    rc_merge_rule R;
    int32_t *rows;              // rc_read_merge
    uint32_t *out_len;          // the plan's: units entries
    const uint32_t *moff;       // the write's: units + 1 entries
    uint8_t *mseq, *mqual;      // mqual may be null
    size_t out_cap;
    unsigned long long *tally;  // may be null
};

__device__ __forceinline__ uint32_t rc_merge_wave_umax(uint32_t x)
{
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)x, sft, 64);
        x = other > x ? other : x;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}

// where the mates of unit u lie and how many of their bases are looked at (both kernels must see the same lengths)
__device__ __forceinline__ void rc_merge_mates(const rc_merge_args &A, uint32_t u, uint32_t lmax, uint32_t (&o)[2], uint32_t (&len)[2])
{
    const uint32_t rd[2] = {A.mode == 2 ? 2u * u : u, A.mode == 2 ? 2u * u + 1u : u + A.units};
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        // (offsets ascend and end inside the arena by contract; ones that do not must still not send a load outside it)
        uint32_t g0 = A.off[rd[mt]];
        const uint32_t g1 = A.off[rd[mt] + 1];
        if (g0 > A.nbytes) g0 = A.nbytes;
        const uint32_t e = g1 > A.nbytes ? A.nbytes : g1;
        const uint32_t l = e > g0 ? e - g0 - 1u : 0u;
        o[mt] = g0;
        len[mt] = l < lmax ? l : lmax;
    }
}

// The offset scan of a pair whose mates are staged in str (a code, a val, room for r code and r val, then mate 2 as read: code,
// val; NW words each): r = the reverse complement of b, then every lane one offset, 64 a round.  Returns the largest key, the
// same in every lane (0: no accepted offset).  The caller has synchronised the wavefront behind the staging.
template <int NW>
__device__ __forceinline__ uint32_t rc_merge_scan_pair(uint64_t *str, int La, int Lb, uint32_t ln, int min_overlap, int max_mismatch_pct)
{
    for (uint32_t t = ln; t < (uint32_t)(2 * NW); t += 64u) {  // item t = word + NW (code / val)
        const uint32_t w = t % NW, what = t / NW;
        str[(2u + what) * NW + w] = rc_ov_rc_word(str + 4u * NW + what * NW, NW, Lb, (int)w, what == 0);
    }
    rc_ov_wave_sync();
    const uint64_t *a_code = str, *a_val = str + NW, *r_code = str + 2 * NW, *r_val = str + 3 * NW;
    const int nwa = (La + 31) >> 5;
    int d_lo, d_hi;
    rc_ov_offsets(La, Lb, min_overlap, d_lo, d_hi);
    uint32_t best = 0;
    for (int d0 = d_lo; d0 <= d_hi; d0 += 64) {
        const int d = d0 + (int)ln;
        if (d <= d_hi) {
            int v, m;
            rc_ov_count(a_code, a_val, nwa, r_code, r_val, NW, d, v, m);
            const uint32_t key = rc_ov_key(v, m, d, min_overlap, max_mismatch_pct);
            best = key > best ? key : best;
        }
    }
    return rc_merge_wave_umax(best);
}

// NW: 64-bit words a mate's strings have
template <int NW>
__global__ __launch_bounds__(RC_MERGE_THREADS) void k_merge_plan(rc_merge_args A)
{
    constexpr uint32_t LMAX = 32 * NW < RC_MERGE_MAX_LEN ? 32 * NW : RC_MERGE_MAX_LEN;
    __shared__ uint64_t s_str[RC_MERGE_WAVES][6 * NW];
    __shared__ uint32_t s_bin[RC_MT_BINS];
    for (uint32_t b = threadIdx.x; b < RC_MT_BINS; b += RC_MERGE_THREADS) s_bin[b] = 0;
    __syncthreads();
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *str = s_str[wv];
    uint32_t *str32 = reinterpret_cast<uint32_t *>(str);
    uint32_t tot[RC_MT_TOOK];
#pragma unroll
    for (int t = 0; t < RC_MT_TOOK; ++t) tot[t] = 0;

    for (uint32_t u = blockIdx.x * RC_MERGE_WAVES + wv; u < A.units; u += gridDim.x * RC_MERGE_WAVES) {
        uint32_t o[2], len[2];
        rc_merge_mates(A, u, LMAX, o, len);
        const int La = (int)len[0], Lb = (int)len[1];
        rc_ov_wave_sync();  // (the last unit's strings are done with)
        // stage: item t = chunk + 2 NW mate
        for (uint32_t t = ln; t < (uint32_t)(4 * NW); t += 64u) {
            const uint32_t c = t % (2u * NW), mt = t / (2u * NW);
            uint32_t code, val;
            rc_ov_chunk(A.seq, mt ? o[1] : o[0], mt ? len[1] : len[0], c, code, val);
            // chunk 2 w is the high half of word w, chunk 2 w + 1 its low half
            const uint32_t base = mt ? 4u * NW : 0u;  // in 64-bit words: b as read / a code
            str32[2u * base + (c ^ 1u)] = code;
            str32[2u * (base + NW) + (c ^ 1u)] = val;
        }
        rc_ov_wave_sync();
        const uint32_t best = rc_merge_scan_pair<NW>(str, La, Lb, ln, A.R.min_overlap, A.R.max_mismatch_pct);
        int F, d, v, m;  // (the same in every lane)
        rc_merge_row(best, Lb, F, d, v, m);
        ++tot[RC_MT_PAIRS];
        tot[RC_MT_MERGED] += best ? 1u : 0u;
        tot[RC_MT_UNMERGED] += best ? 0u : 1u;
        tot[RC_MT_THROUGH] += best && rc_merge_readthrough(La, d, F) ? 1u : 0u;
        tot[RC_MT_COMPARED] += (uint32_t)v;
        tot[RC_MT_MISMATCH] += (uint32_t)m;
        if (ln < 4u) A.rows[4u * (size_t)u + ln] = ln == 0 ? F : ln == 1 ? d : ln == 2 ? v : m;
        if (ln == 4u) {
            A.out_len[u] = (uint32_t)F + 1u;
            atomicAdd(&s_bin[RC_MT_TOTALS + (F & (RC_MERGE_LEN_BINS - 1))], 1u);
        }
    }
    if (!A.tally) return;
    if (ln == 0) {
#pragma unroll
        for (int t = 0; t < RC_MT_TOOK; ++t)
            if (tot[t]) atomicAdd(&s_bin[t], tot[t]);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RC_MT_BINS; b += RC_MERGE_THREADS) {
        const uint32_t v = s_bin[b];
        if (v) atomicAdd(&A.tally[b], (unsigned long long)v);
    }
}

template <int NW>
__global__ __launch_bounds__(RC_MERGE_THREADS) void k_merge_write(rc_merge_args A)
{
    constexpr uint32_t LMAX = 32 * NW < RC_MERGE_MAX_LEN ? 32 * NW : RC_MERGE_MAX_LEN;
    constexpr uint32_t CH = 2 * NW;  // 16-byte chunks a mate's bytes have
    // the bytes of a wavefront's unit: a, qa, b, qb
    __shared__ uint4 s_raw[RC_MERGE_WAVES][4 * CH];
    __shared__ uint32_t s_tk[3];
    if (threadIdx.x < 3) s_tk[threadIdx.x] = 0;
    __syncthreads();
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint4 *raw = s_raw[wv];
    const uint8_t *rawb = reinterpret_cast<const uint8_t *>(raw);
    const bool has_q = A.qual != nullptr;
    uint32_t tk[3] = {0, 0, 0};

    for (uint32_t u = blockIdx.x * RC_MERGE_WAVES + wv; u < A.units; u += gridDim.x * RC_MERGE_WAVES) {
        const int F = __builtin_amdgcn_readfirstlane(A.rows[4u * (size_t)u]);
        const int d = __builtin_amdgcn_readfirstlane(A.rows[4u * (size_t)u + 1u]);
        const size_t beg = A.moff[u], end = A.moff[u + 1u];
        // (what the plan and the scan left: a span of F + 1 bytes inside the arena; anything else is not written)
        if (end > A.out_cap || end < beg || end - beg != (size_t)F + 1u) continue;
        if (F == 0) {
            if (ln == 0) {
                A.mseq[beg] = 0;
                if (A.mqual) A.mqual[beg] = 0;
            }
            continue;
        }
        uint32_t o[2], len[2];
        rc_merge_mates(A, u, LMAX, o, len);
        rc_ov_wave_sync();  // (the last unit's bytes are done with)
        // stage: item t = chunk + CH string; string 2 mate + (0: bases, 1: qualities)
        for (uint32_t t = ln; t < 4u * CH; t += 64u) {
            const uint32_t c = t % CH, s = t / CH, mt = s >> 1;
            if ((s & 1u) && !has_q) continue;
            uint32_t w[4];
            rc_ov_load16((s & 1u) ? A.qual : A.seq, mt ? o[1] : o[0], mt ? len[1] : len[0], c, w);
            raw[s * CH + c] = make_uint4(w[0], w[1], w[2], w[3]);
        }
        rc_ov_wave_sync();
        rc_merge_unit U;
        U.a = rawb;
        U.qa = has_q ? rawb + 16u * CH : nullptr;
        U.b = rawb + 32u * CH;
        U.qb = has_q ? rawb + 48u * CH : nullptr;
        U.La = (int)len[0];
        U.Lb = (int)len[1];
        U.d = d;
        U.F = F;
        const uint32_t lead = (uint32_t)(beg & 15u);  // (d_mseq and d_mqual lie on 16-byte boundaries)
        const uint32_t n_gran = (lead + (uint32_t)F + 1u + 15u) >> 4;
        for (uint32_t g = ln; g < n_gran; g += 64u) {
            uint32_t ws[4], wq[4];
            const uint32_t mask = rc_merge_granule(A.R, U, (int)(16u * g) - (int)lead, ws, wq, tk);
            const size_t at = beg - lead + 16u * (size_t)g;
            if (mask == 0xFFFFu) {
                *reinterpret_cast<uint4 *>(A.mseq + at) = make_uint4(ws[0], ws[1], ws[2], ws[3]);
                if (A.mqual) *reinterpret_cast<uint4 *>(A.mqual + at) = make_uint4(wq[0], wq[1], wq[2], wq[3]);
            } else {
#pragma unroll
                for (int k = 0; k < 16; ++k)
                    if ((mask >> k) & 1u) {
                        A.mseq[at + k] = (uint8_t)(ws[k >> 2] >> (8 * (k & 3)));
                        if (A.mqual) A.mqual[at + k] = (uint8_t)(wq[k >> 2] >> (8 * (k & 3)));
                    }
            }
        }
    }
    if (!A.tally) return;
#pragma unroll
    for (int t = 0; t < 3; ++t)
        if (tk[t]) atomicAdd(&s_tk[t], tk[t]);
    __syncthreads();
    if (threadIdx.x < 3 && s_tk[threadIdx.x]) atomicAdd(&A.tally[RC_MT_TOOK + threadIdx.x], (unsigned long long)s_tk[threadIdx.x]);
}

int rc_launch_read_merge(rc_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int max_read_len,
                         int mode, const void *params, void *d_rows, uint8_t *d_mseq, uint8_t *d_mqual, uint32_t *d_moff, size_t out_cap, void *d_tally)
{
    const rc_merge_params *p = static_cast<const rc_merge_params *>(params);
    const uint32_t units = n_reads >> 1;
    if (units == 0) return RC_OK;
    hipStream_t st = ctx->stream;
    // scratch of the context (the compaction's, free between its passes): the units' lengths, then rocPRIM's
    const size_t n_scan = (size_t)units + 1, len_bytes = (n_scan * 4 + 255) & ~(size_t)255;
    size_t t_scan = 0;
    RC_CHECK_HIP(ctx, rocprim::exclusive_scan(nullptr, t_scan, (uint32_t *)nullptr, (uint32_t *)nullptr, 0u, n_scan, rocprim::plus<uint32_t>(), st));
    if (const int rc = rc_dbuf_reserve(ctx, &ctx->sel_tmp, len_bytes + t_scan + 256)) return rc;
    uint32_t *out_len = static_cast<uint32_t *>(ctx->sel_tmp.p);
    void *scan_tmp = static_cast<uint8_t *>(ctx->sel_tmp.p) + len_bytes;

    rc_merge_args A;
    A.seq = d_seq;
    A.qual = d_qual;
    A.nbytes = (uint32_t)nbytes;
    A.off = d_off;
    A.units = units;
    A.mode = mode;
    A.R.min_overlap = p->min_overlap;
    A.R.max_mismatch_pct = p->max_mismatch_pct;
    A.R.qual_base = p->qual_base;
    A.R.qual_cap = p->qual_cap;
    A.rows = (int32_t *)d_rows;
    A.out_len = out_len;
    A.moff = d_moff;
    A.mseq = d_mseq;
    A.mqual = d_mqual;
    A.out_cap = out_cap;
    A.tally = (unsigned long long *)d_tally;
    // Both kernels read the input arenas in whole aligned 16-byte pieces, as k_mate_overlap does (rc_launch_mate_overlap).
    // Persistent workgroups, a wavefront per unit.  The plan is k_read_trim's pair section and is sized as that kernel is:
    // seven workgroups a CU.  The write holds 4 KB (narrow) or 16 KB (wide) of LDS a workgroup: eight a CU.
    const bool narrow = max_read_len <= 256;
    const unsigned g_all = (units + RC_MERGE_WAVES - 1) / RC_MERGE_WAVES;
    const unsigned g_plan = std::min(g_all, (unsigned)ctx->n_cu * 7u), g_write = std::min(g_all, (unsigned)ctx->n_cu * 8u);
    RC_CHECK_HIP(ctx, hipMemsetAsync(out_len + units, 0, 4, st));
    if (narrow)
        hipLaunchKernelGGL(k_merge_plan<8>, dim3(g_plan), dim3(RC_MERGE_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL(k_merge_plan<32>, dim3(g_plan), dim3(RC_MERGE_THREADS), 0, st, A);
    RC_CHECK_HIP(ctx, hipGetLastError());
    RC_CHECK_HIP(ctx, rocprim::exclusive_scan(scan_tmp, t_scan, out_len, d_moff, 0u, n_scan, rocprim::plus<uint32_t>(), st));
    if (narrow)
        hipLaunchKernelGGL(k_merge_write<8>, dim3(g_write), dim3(RC_MERGE_THREADS), 0, st, A);
    else
        hipLaunchKernelGGL(k_merge_write<32>, dim3(g_write), dim3(RC_MERGE_THREADS), 0, st, A);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
