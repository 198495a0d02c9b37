// rc_overlap.hip -- the mate-overlap report (include/rcorrector_amd.h: rc_mate_overlap; arithmetic in rc_overlap.h): where mate 1
// and the reverse complement of mate 2 cover the same bases, how many of those bases the two disagree on, before and after
// correction.
//
// One launch over two arenas, the snapshot taken before correction and the corrected arena.  A wavefront per pair, persistent
// workgroups striding over the pairs:
//   * stage: lane c takes bytes [16 c, 16 c + 16) of a mate, in ALIGNED 16-byte pieces from the boundary at or in front of the
//     read (k_read_keys' loads: the two pieces a chunk straddles are shifted together, the bytes behind the read's end
//     cleared), packs them with rc_pack16m and stores half a word of the mate's code and validity strings in LDS; both mates
//     of both versions side by side in the lanes of one pass where a mate has up to 256 bases.  Mate 2 is then reversed and
//     complemented word by word (rc_ov_rc_word);
//   * scan: every lane takes one offset d and walks the words of mate 1 -- funnel shift of r, XOR, fold, AND of the validity
//     strings, population counts (rc_ov_count) -- 64 offsets a round; the best offset is the largest 32-bit key (rc_ov_key: v,
//     then the fewest mismatches, then the smallest d), a butterfly of six shuffles.  d* comes from the BEFORE version alone;
//   * classify: lane l takes position 64 j + l of mate 1 at d*, its bit in the faced words of both versions, and adds to the
//     per-position histograms in LDS; the totals are population counts of ballots, kept wave-uniform in registers.
// The histograms live in LDS, 32 bits a bin, laid out as rc_mate_overlap's counts, and every workgroup adds its non-zero bins
// to the caller's 64-bit counts once, at the end (as k_change_report does).  Two instances by the longest read: 8 words a mate
// (up to 256 bases) and 32 (up to RC_OV_MAX_LEN); a mate longer than its instance holds is cut to that, so a wrong
// max_read_len never indexes outside LDS or the arrays.
#include <algorithm>

#include "../../include/rcorrector_amd.h"
#include "rc_internal.h"
#include "rc_overlap.h"
#include "rc_overlap_stage.h"  // rc_ov_wave_sync, rc_ov_chunk

#define RC_OV_THREADS 256
#define RC_OV_WAVES (RC_OV_THREADS / 64)
// 64-bit words of rc_mate_overlap in front of its counts (min_overlap, max_mismatch_pct), the twelve totals, and the bins
#define RC_OV_HEAD 2
#define RC_OV_TOTALS 12
#define RC_OV_BINS (RC_OV_TOTALS + RC_OV_FRAG + 6 * RC_OV_POS)
static_assert(sizeof(rc_mate_overlap) == (RC_OV_HEAD + RC_OV_BINS) * 8, "the bins are an rc_mate_overlap's counts");
static_assert(RC_OV_FRAG == RC_OVERLAP_FRAG_LEN && RC_OV_POS == RC_OVERLAP_MAX_LEN, "rc_overlap.h's sizes are the header's");
enum {
    RC_OV_PAIRS = 0, RC_OV_OVERLAPPING, RC_OV_CMP_B, RC_OV_DIS_B, RC_OV_CMP_A, RC_OV_DIS_A, RC_OV_RESOLVED, RC_OV_INTRODUCED, RC_OV_KEPT,
    RC_OV_IMPROVED, RC_OV_WORSENED, RC_OV_SAME,
    RC_OV_BIN_FRAG = RC_OV_TOTALS,
    RC_OV_BIN_CMP5 = RC_OV_BIN_FRAG + RC_OV_FRAG,
    RC_OV_BIN_DISB5 = RC_OV_BIN_CMP5 + 2 * RC_OV_POS,
    RC_OV_BIN_DISA5 = RC_OV_BIN_DISB5 + 2 * RC_OV_POS
};

struct rc_overlap_args {
    const uint8_t *ver[2];  // the arena before / after correction (may be one and the same)
    uint32_t nbytes;
    const uint32_t *off;
    uint32_t pairs;
    int mode;  // 1 or 2
    int min_overlap, max_mismatch_pct;
    unsigned long long *out;  // an rc_mate_overlap
};

// NW: 64-bit words a mate's strings have
template <int NW>
__global__ __launch_bounds__(RC_OV_THREADS) void k_mate_overlap(rc_overlap_args A)
{
    constexpr uint32_t LMAX = 32 * NW < RC_OV_MAX_LEN ? 32 * NW : RC_OV_MAX_LEN;
    // strings of a wavefront's pair: [version][a code, a val, r code, r val][NW], then mate 2 as read: [version][code, val][NW]
    __shared__ uint64_t s_str[RC_OV_WAVES][12 * NW];
    __shared__ uint32_t s_bin[RC_OV_BINS];
    for (uint32_t b = threadIdx.x; b < RC_OV_BINS; b += RC_OV_THREADS) s_bin[b] = 0;
    __syncthreads();
    const uint32_t ln = threadIdx.x & 63u;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    uint64_t *str = s_str[wv];
    uint32_t *str32 = reinterpret_cast<uint32_t *>(str);
    const bool same = A.ver[0] == A.ver[1];
    const int n_ver = same ? 1 : 2;
    uint32_t tot[RC_OV_TOTALS];
#pragma unroll
    for (int t = 0; t < RC_OV_TOTALS; ++t) tot[t] = 0;

    for (uint32_t u = blockIdx.x * RC_OV_WAVES + wv; u < A.pairs; u += gridDim.x * RC_OV_WAVES) {
        const uint32_t rd[2] = {A.mode == 1 ? u : 2u * u, A.mode == 1 ? u + A.pairs : 2u * u + 1u};
        uint32_t o[2], len[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
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
        ++tot[RC_OV_PAIRS];
        rc_ov_wave_sync();  // (the last pair's strings are done with)
        // stage: item t = chunk + 2 NW (mate + 2 version)
        for (uint32_t t = ln; t < (uint32_t)(4 * NW * n_ver); t += 64u) {
            const uint32_t c = t % (2u * NW), mt = (t / (2u * NW)) & 1u, vr = t / (4u * NW);
            uint32_t code, val;
            rc_ov_chunk(A.ver[vr], mt ? o[1] : o[0], mt ? len[1] : len[0], c, code, val);
            // chunk 2 w is the high half of word w, chunk 2 w + 1 its low half
            const uint32_t base = mt ? (8u * NW + vr * 2u * NW) : vr * 4u * NW;  // in 64-bit words: b as read / a code
            str32[2u * base + (c ^ 1u)] = code;
            str32[2u * (base + NW) + (c ^ 1u)] = val;
        }
        rc_ov_wave_sync();
        // r = reverse complement of b: item t = word + NW (code / val + 2 version)
        for (uint32_t t = ln; t < (uint32_t)(2 * NW * n_ver); t += 64u) {
            const uint32_t w = t % NW, what = (t / NW) & 1u, vr = t / (2u * NW);
            const uint64_t *b_str = str + 8u * NW + vr * 2u * NW + what * NW;
            str[vr * 4u * NW + (2u + what) * NW + w] = rc_ov_rc_word(b_str, NW, Lb, (int)w, what == 0);
        }
        rc_ov_wave_sync();
        const uint64_t *a_code = str, *a_val = str + NW, *r_code = str + 2 * NW, *r_val = str + 3 * NW;
        const int nwa = (La + 31) >> 5;
        // scan the offsets of the BEFORE version
        int d_lo, d_hi;
        rc_ov_offsets(La, Lb, A.min_overlap, d_lo, d_hi);
        uint32_t best = 0;
        for (int d0 = d_lo; d0 <= d_hi; d0 += 64) {
            const int d = d0 + (int)ln;
            if (d <= d_hi) {
                int v, m;
                rc_ov_count(a_code, a_val, nwa, r_code, r_val, NW, d, v, m);
                const uint32_t key = rc_ov_key(v, m, d, A.min_overlap, A.max_mismatch_pct);
                best = key > best ? key : best;
            }
        }
#pragma unroll
        for (int sft = 32; sft > 0; sft >>= 1) {
            const uint32_t other = (uint32_t)__shfl_xor((int)best, sft, 64);
            best = other > best ? other : best;
        }
        best = (uint32_t)__builtin_amdgcn_readfirstlane((int)best);
        if (best == 0) continue;  // (the same in every lane) not overlapping
        const int ds = rc_ov_key_d(best);
        // classify the positions of a at d*, in both versions
        const uint64_t *c_code = str + (same ? 0 : 4 * NW), *c_val = c_code + NW, *q_code = c_code + 2 * NW, *q_val = c_code + 3 * NW;
        uint32_t cb = 0, db = 0, ca = 0, da = 0;
        for (int i0 = 0; i0 < La; i0 += 64) {
            const int i = i0 + (int)ln, w = i >> 5;  // (i < 32 NW: La <= LMAX)
            const rc_ov_faced fb = rc_ov_face(a_code, a_val, r_code, r_val, NW, ds, w);
            const rc_ov_faced fa = rc_ov_face(c_code, c_val, q_code, q_val, NW, ds, w);
            const uint64_t bit = rc_ov_bit(i);
            const bool vb = (fb.both & bit) != 0, xb = (fb.differ & bit) != 0, va = (fa.both & bit) != 0, xa = (fa.differ & bit) != 0;
            // (a faced position: 0 <= i - ds < Lb, so p2 is a position of b; RC_OV_POS - 1 bounds both all the same)
            const uint32_t p1 = (uint32_t)i & (RC_OV_POS - 1), p2 = (uint32_t)(Lb - 1 - (i - ds)) & (RC_OV_POS - 1);
            if (vb) {
                atomicAdd(&s_bin[RC_OV_BIN_CMP5 + p1], 1u);
                atomicAdd(&s_bin[RC_OV_BIN_CMP5 + RC_OV_POS + p2], 1u);
            }
            if (xb) {
                atomicAdd(&s_bin[RC_OV_BIN_DISB5 + p1], 1u);
                atomicAdd(&s_bin[RC_OV_BIN_DISB5 + RC_OV_POS + p2], 1u);
            }
            if (xa) {
                atomicAdd(&s_bin[RC_OV_BIN_DISA5 + p1], 1u);
                atomicAdd(&s_bin[RC_OV_BIN_DISA5 + RC_OV_POS + p2], 1u);
            }
            cb += (uint32_t)__popcll(__ballot(vb));
            db += (uint32_t)__popcll(__ballot(xb));
            ca += (uint32_t)__popcll(__ballot(va));
            da += (uint32_t)__popcll(__ballot(xa));
            tot[RC_OV_RESOLVED] += (uint32_t)__popcll(__ballot(xb && va && !xa));
            tot[RC_OV_INTRODUCED] += (uint32_t)__popcll(__ballot(vb && !xb && xa));
            tot[RC_OV_KEPT] += (uint32_t)__popcll(__ballot(xb && xa));
        }
        ++tot[RC_OV_OVERLAPPING];
        tot[RC_OV_CMP_B] += cb;
        tot[RC_OV_DIS_B] += db;
        tot[RC_OV_CMP_A] += ca;
        tot[RC_OV_DIS_A] += da;
        tot[RC_OV_IMPROVED] += da < db ? 1u : 0u;  // (no run-time index: the totals stay in registers)
        tot[RC_OV_WORSENED] += da > db ? 1u : 0u;
        tot[RC_OV_SAME] += da == db ? 1u : 0u;
        if (ln == 0) atomicAdd(&s_bin[RC_OV_BIN_FRAG + ((uint32_t)(ds + Lb) & (RC_OV_FRAG - 1))], 1u);
    }
    if (ln == 0) {
#pragma unroll
        for (int t = 0; t < RC_OV_TOTALS; ++t)
            if (tot[t]) atomicAdd(&s_bin[t], tot[t]);
    }
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RC_OV_BINS; b += RC_OV_THREADS) {
        const uint32_t v = s_bin[b];
        if (v) atomicAdd(&A.out[RC_OV_HEAD + b], (unsigned long long)v);
    }
}

int rc_launch_mate_overlap(rc_ctx *ctx, const uint8_t *d_before, const uint8_t *d_after, size_t nbytes, const uint32_t *d_off, uint32_t n_reads,
                           int max_read_len, int mode, int min_overlap, int max_mismatch_pct, void *d_counts)
{
    const uint32_t pairs = n_reads >> 1;
    if (pairs == 0) return RC_OK;
    rc_overlap_args A;
    A.ver[0] = d_before;
    A.ver[1] = d_after;
    A.nbytes = (uint32_t)nbytes;
    A.off = d_off;
    A.pairs = pairs;
    A.mode = mode;
    A.min_overlap = min_overlap;
    A.max_mismatch_pct = max_mismatch_pct;
    A.out = (unsigned long long *)d_counts;
    // The kernel reads both arenas in whole aligned 16-byte pieces: up to 15 bytes in front of an arena and behind its last read
    // are loaded and shifted or masked off.  An aligned 16-byte piece that holds one byte of an arena lies in that byte's page, so
    // the loads cannot fault; an allocator or checker that is exact to the byte would have to know.
    // Persistent workgroups, a wavefront per pair: the narrow instance's 36 KB of LDS let four of them share a CU, the wide
    // one's 45 KB three.
    const bool narrow = max_read_len <= 256;
    unsigned g = (pairs + RC_OV_WAVES - 1) / RC_OV_WAVES;
    g = std::min(g, (unsigned)ctx->n_cu * (narrow ? 4u : 3u));
    if (narrow)
        hipLaunchKernelGGL(k_mate_overlap<8>, dim3(g), dim3(RC_OV_THREADS), 0, ctx->stream, A);
    else
        hipLaunchKernelGGL(k_mate_overlap<32>, dim3(g), dim3(RC_OV_THREADS), 0, ctx->stream, A);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
