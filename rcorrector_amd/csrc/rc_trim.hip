// rc_trim.hip -- read trimming (include/rcorrector_amd.h: rc_read_trim_device; the contract in rc_trim.h): per read, how many
// bases to keep after a 3' quality cut, a 3' adapter cut and, for pairs, the cut of a mate that ran through its fragment.
//
// Shaped as k_mate_overlap (rc_overlap.hip): a wavefront per unit -- a read, or a pair -- persistent workgroups striding over
// the units:
//   * stage: lane c takes bytes [16 c, 16 c + 16) of a mate in aligned 16-byte pieces (rc_ov_chunk) and stores half a word of
//     the mate's code and validity strings in LDS, both mates side by side in the lanes;
//   * pair cut: mate 2 reversed and complemented word by word, then every lane one offset d, 64 a round, the largest rc_ov_key
//     by a butterfly of shuffles -- k_mate_overlap's scan of the BEFORE version, token for token;
//   * adapter cut: every lane one offset d of the mate against its adapter's strings (rc_trim_ad_count), 64 a round in
//     ascending order: the first round with an accepted offset ends the scan, its lowest lane is the cut (one ballot);
//   * quality cut: lane c takes bytes [16 c, 16 c + 16) of the quality string with the same wide loads, 16 lane-local suffix
//     sums, a suffix scan of the lanes' totals (six shuffles), one max-reduction for i0 and one for the best key.
// The per-unit values are wave-uniform and counted in registers; the length histograms live in LDS, 32 bits a bin, and every
// workgroup adds its non-zero bins to the caller's 64-bit tally once, at the end.  Two instances by the longest read: 8 words a
// mate (up to 256 bases) and 32 (up to RC_TRIM_MAX_LEN); a mate longer than its instance holds is cut to that, so a wrong
// max_read_len never indexes outside LDS.
#include <algorithm>
#include <cstddef>

#include "../../include/rcorrector_amd.h"
#include "rc_internal.h"
#include "rc_overlap_stage.h"
#include "rc_trim.h"

#define RC_TRIM_THREADS 256
#define RC_TRIM_WAVES (RC_TRIM_THREADS / 64)
// the 64-bit words of an rc_trim_tally: fifteen totals, then keep_hist
enum {
    RC_TT_READS = 0, RC_TT_CUT = 2, RC_TT_REMOVED = 8, RC_TT_SHORT = 10, RC_TT_UNITS = 12, RC_TT_KEPT = 13, RC_TT_OVL = 14,
    RC_TT_TOTALS = 15,
    RC_TT_BINS = RC_TT_TOTALS + 2 * 1024
};
static_assert(sizeof(rc_trim_tally) == RC_TT_BINS * 8, "the bins are an rc_trim_tally");
static_assert(offsetof(rc_trim_tally, cut_reads) == RC_TT_CUT * 8 && offsetof(rc_trim_tally, bases_removed) == RC_TT_REMOVED * 8 &&
                  offsetof(rc_trim_tally, short_reads) == RC_TT_SHORT * 8 && offsetof(rc_trim_tally, units) == RC_TT_UNITS * 8 &&
                  offsetof(rc_trim_tally, units_kept) == RC_TT_KEPT * 8 && offsetof(rc_trim_tally, pairs_overlapping) == RC_TT_OVL * 8 &&
                  offsetof(rc_trim_tally, keep_hist) == RC_TT_TOTALS * 8,
              "as k_read_trim indexes them");
static_assert(sizeof(rc_read_trim) == 16, "16 bytes per read");

struct rc_trim_args {
    const uint8_t *seq, *qual;  // qual may be null
    uint32_t nbytes;
    const uint32_t *off;
    uint32_t units;
    int mode;
    int qual_min, qual_base, adapter_min, adapter_mm_pct, pair_overlap, pair_min_overlap, pair_mm_pct, min_len;
    int ad_len[2];
    uint64_t ad[2][2 * RC_TRIM_AD_WORDS];  // per mate: the adapter's code words, then its validity words
    int32_t *out;                          // rc_read_trim rows
    uint8_t *keep;                         // may be null
    unsigned long long *tally;             // may be null
};

__device__ __forceinline__ int rc_trim_wave_max(int x)
{
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        const int other = __shfl_xor(x, sft, 64);
        x = other > x ? other : x;
    }
    return __builtin_amdgcn_readfirstlane(x);
}
__device__ __forceinline__ uint32_t rc_trim_wave_umax(uint32_t x)
{
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) {
        const uint32_t other = (uint32_t)__shfl_xor((int)x, sft, 64);
        x = other > x ? other : x;
    }
    return (uint32_t)__builtin_amdgcn_readfirstlane((int)x);
}

// NW: 64-bit words a mate's strings have
template <int NW>
__global__ __launch_bounds__(RC_TRIM_THREADS) void k_read_trim(rc_trim_args A)
{
    constexpr uint32_t LMAX = 32 * NW < RC_TRIM_MAX_LEN ? 32 * NW : RC_TRIM_MAX_LEN;
    // strings of a wavefront's unit: a code, a val, r code, r val, then mate 2 as read: code, val
    __shared__ uint64_t s_str[RC_TRIM_WAVES][6 * NW];
    __shared__ uint64_t s_ad[2][2 * RC_TRIM_AD_WORDS];
    __shared__ uint32_t s_bin[RC_TT_BINS];
    for (uint32_t b = threadIdx.x; b < RC_TT_BINS; b += RC_TRIM_THREADS) s_bin[b] = 0;
    if (threadIdx.x < 4 * RC_TRIM_AD_WORDS) s_ad[threadIdx.x / (2 * RC_TRIM_AD_WORDS)][threadIdx.x % (2 * RC_TRIM_AD_WORDS)] =
        A.ad[threadIdx.x / (2 * RC_TRIM_AD_WORDS)][threadIdx.x % (2 * RC_TRIM_AD_WORDS)];
    __syncthreads();
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *str = s_str[wv];
    uint32_t *str32 = reinterpret_cast<uint32_t *>(str);
    const int n_mates = A.mode == 0 ? 1 : 2;
    const bool do_qual = A.qual != nullptr && A.qual_min > 0;
    uint32_t tot[RC_TT_TOTALS];
#pragma unroll
    for (int t = 0; t < RC_TT_TOTALS; ++t) tot[t] = 0;

    for (uint32_t u = blockIdx.x * RC_TRIM_WAVES + wv; u < A.units; u += gridDim.x * RC_TRIM_WAVES) {
        const uint32_t rd[2] = {A.mode == 2 ? 2u * u : u, A.mode == 2 ? 2u * u + 1u : (A.mode == 1 ? u + A.units : u)};
        uint32_t o[2] = {0, 0}, len[2] = {0, 0};
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (mt >= n_mates) break;
            // (offsets ascend and end inside the arena by contract; ones that do not must still not send a load outside it)
            uint32_t g0 = A.off[rd[mt]];
            const uint32_t g1 = A.off[rd[mt] + 1];
            if (g0 > A.nbytes) g0 = A.nbytes;
            const uint32_t e = g1 > A.nbytes ? A.nbytes : g1;
            const uint32_t l = e > g0 ? e - g0 - 1u : 0u;
            o[mt] = g0;
            len[mt] = l < LMAX ? l : LMAX;
        }
        const int La = (int)len[0], Lb = (int)len[1];
        rc_ov_wave_sync();  // (the last unit's strings are done with)
        // stage: item t = chunk + 2 NW mate
        for (uint32_t t = ln; t < (uint32_t)(2 * NW * n_mates); t += 64u) {
            const uint32_t c = t % (2u * NW), mt = t / (2u * NW);
            uint32_t code, val;
            rc_ov_chunk(A.seq, mt ? o[1] : o[0], mt ? len[1] : len[0], c, code, val);
            // chunk 2 w is the high half of word w, chunk 2 w + 1 its low half
            const uint32_t base = mt ? 4u * NW : 0u;  // in 64-bit words: b as read / a code
            str32[2u * base + (c ^ 1u)] = code;
            str32[2u * (base + NW) + (c ^ 1u)] = val;
        }
        rc_ov_wave_sync();
        const uint64_t *a_code = str, *a_val = str + NW, *r_code = str + 2 * NW, *r_val = str + 3 * NW;
        int cut_q[2] = {La, Lb}, cut_ad[2] = {La, Lb}, cut_pair[2] = {La, Lb};

        // the pair cut: k_mate_overlap's choice of d*
        if (n_mates == 2 && A.pair_overlap) {
            for (uint32_t t = ln; t < (uint32_t)(2 * NW); t += 64u) {  // r = reverse complement of b: item t = word + NW (code / val)
                const uint32_t w = t % NW, what = t / NW;
                str[(2u + what) * NW + w] = rc_ov_rc_word(str + 4u * NW + what * NW, NW, Lb, (int)w, what == 0);
            }
            rc_ov_wave_sync();
            const int nwa = (La + 31) >> 5;
            int d_lo, d_hi;
            rc_ov_offsets(La, Lb, A.pair_min_overlap, d_lo, d_hi);
            uint32_t best = 0;
            for (int d0 = d_lo; d0 <= d_hi; d0 += 64) {
                const int d = d0 + (int)ln;
                if (d <= d_hi) {
                    int v, m;
                    rc_ov_count(a_code, a_val, nwa, r_code, r_val, NW, d, v, m);
                    const uint32_t key = rc_ov_key(v, m, d, A.pair_min_overlap, A.pair_mm_pct);
                    best = key > best ? key : best;
                }
            }
            best = rc_trim_wave_umax(best);
            if (best != 0) {  // (the same in every lane)
                rc_trim_pair_cuts(La, Lb, rc_ov_key_d(best), cut_pair[0], cut_pair[1]);
                ++tot[RC_TT_OVL];
            }
        }

#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (mt >= n_mates) break;
            const int L = (int)len[mt];
            // the adapter cut: the smallest accepted offset
            if (A.ad_len[mt] > 0) {
                const uint64_t *m_code = str + (mt ? 4 * NW : 0), *m_val = m_code + NW;
                const int nw = (L + 31) >> 5;
                for (int d0 = 0; d0 < L; d0 += 64) {
                    const int d = d0 + (int)ln;
                    bool ok = false;
                    if (d < L) {
                        int v, m;
                        rc_trim_ad_count(m_code, m_val, nw, s_ad[mt], s_ad[mt] + RC_TRIM_AD_WORDS, d, v, m);
                        ok = rc_trim_ad_accepts(v, m, A.adapter_min, A.adapter_mm_pct);
                    }
                    const unsigned long long hit = __ballot(ok);
                    if (hit) {  // (the same in every lane)
                        cut_ad[mt] = d0 + __ffsll((long long)hit) - 1;
                        break;
                    }
                }
            }
            // the quality cut
            if (do_qual) {
                const int pos0 = 16 * (int)ln;
                const int left = L - pos0 < 0 ? 0 : (L - pos0 > 16 ? 16 : L - pos0);
                uint32_t w[4];
                rc_ov_load16(A.qual, o[mt], (uint32_t)L, ln, w);
                int suf[16];
                rc_trim_qual_suffix(w, left, A.qual_min, A.qual_base, suf);
                int incl = suf[0];  // -> the sum over this lane and the lanes behind it
#pragma unroll
                for (int sft = 1; sft < 64; sft <<= 1) {
                    const int other = __shfl_down(incl, sft, 64);
                    if (ln + (uint32_t)sft < 64u) incl += other;
                }
                const int behind = incl - suf[0];
                const int i0 = rc_trim_wave_max(rc_trim_qual_neg(suf, behind, left, pos0));
                const uint32_t at_end = rc_trim_qual_key(0, L);
                uint32_t best = rc_trim_wave_umax(rc_trim_qual_best(suf, behind, left, pos0, i0));
                best = at_end > best ? at_end : best;
                cut_q[mt] = rc_trim_qual_key_pos(best);
            }
        }

        int keep_len[2] = {0, 0};
        bool kept = true;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            if (mt >= n_mates) break;
            const int L = (int)len[mt];
            keep_len[mt] = rc_trim_keep_len(cut_q[mt], cut_ad[mt], cut_pair[mt]);
            kept = kept && keep_len[mt] >= A.min_len;
            ++tot[RC_TT_READS + mt];
            tot[RC_TT_CUT + 3 * mt + 0] += cut_q[mt] < L ? 1u : 0u;
            tot[RC_TT_CUT + 3 * mt + 1] += cut_ad[mt] < L ? 1u : 0u;
            tot[RC_TT_CUT + 3 * mt + 2] += cut_pair[mt] < L ? 1u : 0u;
            tot[RC_TT_REMOVED + mt] += (uint32_t)(L - keep_len[mt]);
            tot[RC_TT_SHORT + mt] += keep_len[mt] < A.min_len ? 1u : 0u;
        }
        ++tot[RC_TT_UNITS];
        tot[RC_TT_KEPT] += kept ? 1u : 0u;
        // the rows: lane 4 mt + f holds field f of mate mt
        if (ln < (uint32_t)(4 * n_mates)) {
            const int mt = (int)(ln >> 2), f = (int)(ln & 3u);
            const int kl = mt ? keep_len[1] : keep_len[0], cq = mt ? cut_q[1] : cut_q[0], ca = mt ? cut_ad[1] : cut_ad[0], cp = mt ? cut_pair[1] : cut_pair[0];
            A.out[4u * (size_t)(mt ? rd[1] : rd[0]) + (uint32_t)f] = f == 0 ? kl : f == 1 ? cq : f == 2 ? ca : cp;
            if (f == 0) atomicAdd(&s_bin[RC_TT_TOTALS + 1024 * mt + (kl & 1023)], 1u);
        }
        if (ln == 0 && A.keep) A.keep[u] = kept ? 1 : 0;
    }
    if (!A.tally) return;
    if (ln == 0) {
#pragma unroll
        for (int t = 0; t < RC_TT_TOTALS; ++t)
            if (tot[t]) atomicAdd(&s_bin[t], tot[t]);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RC_TT_BINS; b += RC_TRIM_THREADS) {
        const uint32_t v = s_bin[b];
        if (v) atomicAdd(&A.tally[b], (unsigned long long)v);
    }
}

int rc_launch_read_trim(rc_ctx *ctx, const uint8_t *d_seq, const uint8_t *d_qual, size_t nbytes, const uint32_t *d_off, uint32_t n_reads, int max_read_len,
                        int mode, const void *params, void *d_out, uint8_t *d_keep, void *d_tally)
{
    const rc_trim_params *p = static_cast<const rc_trim_params *>(params);
    const uint32_t units = mode == 0 ? n_reads : n_reads >> 1;
    if (units == 0) return RC_OK;
    rc_trim_args A;
    A.seq = d_seq;
    A.qual = d_qual;
    A.nbytes = (uint32_t)nbytes;
    A.off = d_off;
    A.units = units;
    A.mode = mode;
    A.qual_min = p->qual_min;
    A.qual_base = p->qual_base;
    A.adapter_min = p->adapter_min;
    A.adapter_mm_pct = p->adapter_mm_pct;
    A.pair_overlap = p->pair_overlap;
    A.pair_min_overlap = p->pair_min_overlap;
    A.pair_mm_pct = p->pair_mm_pct;
    A.min_len = p->min_len;
    A.ad_len[0] = p->adapter1_len;
    A.ad_len[1] = p->adapter2_len;
    if (!rc_trim_pack_adapter(p->adapter1, p->adapter1_len, A.ad[0], A.ad[0] + RC_TRIM_AD_WORDS) ||
        !rc_trim_pack_adapter(p->adapter2, p->adapter2_len, A.ad[1], A.ad[1] + RC_TRIM_AD_WORDS))
        return RC_ERR_ARG;  // (rc_read_trim_device has said why)
    A.out = (int32_t *)d_out;
    A.keep = d_keep;
    A.tally = (unsigned long long *)d_tally;
    // The kernel reads both arenas in whole aligned 16-byte pieces, as k_mate_overlap does (rc_launch_mate_overlap).
    // Persistent workgroups, a wavefront per unit: 10 KB of LDS in the narrow instance and 15 KB in the wide one, so the
    // registers (65 to 67 a lane: seven waves a SIMD) set the seven workgroups a CU holds.
    const bool narrow = max_read_len <= 256;
    unsigned g = (units + RC_TRIM_WAVES - 1) / RC_TRIM_WAVES;
    g = std::min(g, (unsigned)ctx->n_cu * 7u);
    if (narrow)
        hipLaunchKernelGGL(k_read_trim<8>, dim3(g), dim3(RC_TRIM_THREADS), 0, ctx->stream, A);
    else
        hipLaunchKernelGGL(k_read_trim<32>, dim3(g), dim3(RC_TRIM_THREADS), 0, ctx->stream, A);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
