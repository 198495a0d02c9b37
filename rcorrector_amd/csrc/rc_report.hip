// rc_report.hip -- the correction report (include/rcorrector_amd.h: rc_change_report): every read of a batch arena compared
// with the copy taken before the first correction kernel, the differences counted by position, substitution, quality class,
// mate and read.
//
// A correction only ever writes one of ACGT over a different byte (ErrorCorrection.cpp:1468-1479; k_fix_list_bytes relies
// on the same), so every byte that differs is one change.  Changes are sparse -- about 0.75 per 150-base read at 0.5 %
// errors -- so the kernel is a streaming comparison of two arenas with rare histogram updates:
//   * a quarter wave (16 lanes) per read, 16 bytes per lane and step: a 150-base read is one step of ten or eleven lanes
//     (the house shape, rc_quarter.h: a wavefront per read would idle 54 lanes);
//   * reads start at any alignment, and the snapshot is placed so that it has the arena's alignment (rc_report_snapshot):
//     both sides are read as ALIGNED 16-byte pieces and the bytes outside the read are masked off -- the reads of a launch do
//     not share one shift, which is what rc_load16_any's uniform branch needs;
//   * the histograms live in LDS, 32 bits per bin, per workgroup; a bounded number of persistent workgroups stride over the
//     reads and each adds its non-zero bins to the 64-bit accumulator once, at the end (as k_spectrum_* do);
//   * what every read contributes -- its length, its mate, "no change" -- is kept in registers as a run (reads of one length
//     follow each other) and reaches LDS when the run breaks.
#include "../../include/rcorrector_amd.h"
#include "rc_internal.h"
#include "rc_device.h"

#define RC_REP_THREADS 512
#define RC_REP_QUARTERS (RC_REP_THREADS / 16)

// index of a field in the accumulator, in 64-bit words: the layout of rc_change_report
#define RC_REP_READS 0
#define RC_REP_CHANGED 2
#define RC_REP_UNFIX 4
#define RC_REP_CHANGES 6
#define RC_REP_LEN 8
#define RC_REP_POS5 (RC_REP_LEN + 2 * RC_REPORT_MAX_LEN)
#define RC_REP_POS3 (RC_REP_POS5 + 2 * RC_REPORT_MAX_LEN)
#define RC_REP_SUBST (RC_REP_POS3 + 2 * RC_REPORT_MAX_LEN)
#define RC_REP_QUAL (RC_REP_SUBST + 20)
#define RC_REP_PER_READ (RC_REP_QUAL + 3)
static_assert(RC_REP_PER_READ + RC_REPORT_MAX_PER_READ + 1 == RC_REPORT_WORDS, "the accumulator is an rc_change_report");
static_assert(sizeof(rc_change_report) == RC_REPORT_WORDS * 8, "the accumulator is an rc_change_report");

struct rc_report_args {
    const uint8_t *seq;   // the corrected arena
    ptrdiff_t snap_delta; // the snapshot's byte p lies at seq + p + snap_delta (a multiple of 16)
    const uint32_t *off;
    const int32_t *ret;
    const uint8_t *qual;
    int qual_bits;
    uint32_t qual_split, qual_base2;
    int bad_qual;
    int mode;
    uint32_t n;
    unsigned long long *out;  // RC_REPORT_WORDS
};

__device__ __forceinline__ int rc_rep_letter(uint32_t c) { return c == 0x41u ? 0 : (c == 0x43u ? 1 : (c == 0x47u ? 2 : (c == 0x54u ? 3 : 4))); }

__global__ __launch_bounds__(RC_REP_THREADS) void k_change_report(rc_report_args A)
{
    __shared__ uint32_t s_bin[RC_REPORT_WORDS];
    for (uint32_t b = threadIdx.x; b < RC_REPORT_WORDS; b += RC_REP_THREADS) s_bin[b] = 0;
    __syncthreads();
    const uint32_t l16 = threadIdx.x & 15u, qw = threadIdx.x >> 4;
    const uint32_t n_quarters = gridDim.x * RC_REP_QUARTERS, q = blockIdx.x * RC_REP_QUARTERS + qw;
    const uint32_t iters = (A.n + n_quarters - 1) / n_quarters;  // (the same for every lane: the shuffles below need whole wavefronts)
    const uint32_t half = A.n >> 1;
    // the run of reads of one mate and length that this quarter is in (lane 0 of the quarter keeps it)
    uint32_t run_key = 0xFFFFFFFFu, run_n = 0, run_clean = 0;
    auto flush_run = [&]() {
        if (run_n && l16 == 0) {
            const uint32_t mate = run_key >> 10, len = run_key & 1023u;
            atomicAdd(&s_bin[RC_REP_READS + mate], run_n);
            atomicAdd(&s_bin[RC_REP_LEN + mate * RC_REPORT_MAX_LEN + len], run_n);
            if (run_clean) atomicAdd(&s_bin[RC_REP_PER_READ], run_clean);
        }
        run_n = run_clean = 0;
    };
    uint32_t r = q;
    uint32_t o = 0, o1 = 0;
    if (r < A.n) {
        o = A.off[r];
        o1 = A.off[r + 1];
    }
    for (uint32_t it = 0; it < iters; ++it) {
        const bool live = r < A.n;
        const uint32_t len = live ? o1 - o - 1u : 0u;
        const int32_t rt = live && l16 == 0 ? A.ret[r] : 0;
        const uint32_t rn = r + n_quarters;  // the next read's offsets are on their way while this one is compared
        uint32_t no = 0, no1 = 0;
        if (rn < A.n && it + 1 < iters) {
            no = A.off[rn];
            no1 = A.off[rn + 1];
        }
        const uint32_t mate = A.mode == 0 ? 0u : (A.mode == 1 ? (r >= half ? 1u : 0u) : (r & 1u));
        // aligned 16-byte pieces [a0 + 16 c, ...) that cover the read's bytes [s, s + len)
        const uintptr_t s = (uintptr_t)(A.seq + o), a0 = s & ~(uintptr_t)15;
        const uint32_t lead = (uint32_t)(s - a0), n_pc = live ? (lead + len + 15u) >> 4 : 0u;
        uint32_t mine = 0;
        for (uint32_t c = l16; __any(c < n_pc); c += 16) {  // (every lane of the wavefront stays in the loop until all are done)
            uint32_t d = 0;
            uint4 sv = make_uint4(0, 0, 0, 0), ov = sv;
            if (c < n_pc) {
                const uint8_t *pa = reinterpret_cast<const uint8_t *>(a0 + (uintptr_t)16 * c);
                sv = *reinterpret_cast<const uint4 *>(pa);
                ov = *reinterpret_cast<const uint4 *>(pa + A.snap_delta);
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
            mine += (uint32_t)__popc(d);
            while (d) {
                const int j = __ffs((int)d) - 1;
                d &= d - 1;
                // (selected without indexing the arrays at run time: that would put them into scratch memory)
                const uint32_t wn = j < 8 ? (j < 4 ? sw[0] : sw[1]) : (j < 12 ? sw[2] : sw[3]);
                const uint32_t wo = j < 8 ? (j < 4 ? ow[0] : ow[1]) : (j < 12 ? ow[2] : ow[3]);
                const uint32_t cn = (wn >> (8 * (j & 3))) & 0xffu, co = (wo >> (8 * (j & 3))) & 0xffu;
                const uint32_t pos = (uint32_t)(j - first);
                const uint32_t p5 = pos < RC_REPORT_MAX_LEN - 1 ? pos : RC_REPORT_MAX_LEN - 1;
                const uint32_t p3 = len - 1u - pos < RC_REPORT_MAX_LEN - 1 ? len - 1u - pos : RC_REPORT_MAX_LEN - 1;
                atomicAdd(&s_bin[RC_REP_POS5 + mate * RC_REPORT_MAX_LEN + p5], 1u);
                atomicAdd(&s_bin[RC_REP_POS3 + mate * RC_REPORT_MAX_LEN + p3], 1u);
                // (a correction writes one of ACGT, ErrorCorrection.cpp:1468-1479: the new letter's code is 0..3; the mask only
                // keeps a byte that broke that rule inside the table -- it would be counted as "to A")
                atomicAdd(&s_bin[RC_REP_SUBST + 4 * rc_rep_letter(co) + (rc_rep_letter(cn) & 3)], 1u);
                // the correction's own tests (rc_correct_core.h: q0 != 0 is the FASTQ marker, qual <= badQualityThreshold is low)
                const int q0 = (int)rc_qual_at(A.qual, A.qual_bits, A.qual_split, A.qual_base2, o);
                const int qp = (int)rc_qual_at(A.qual, A.qual_bits, A.qual_split, A.qual_base2, o + pos);
                atomicAdd(&s_bin[RC_REP_QUAL + (q0 == 0 ? 2 : (qp <= A.bad_qual ? 0 : 1))], 1u);
            }
        }
        // the read's changes: the sum over its quarter
        uint32_t tot = mine;
        if (__any(mine != 0)) {
#pragma unroll
            for (int sft = 1; sft < 16; sft <<= 1) tot += __shfl_xor(tot, sft, 16);
        }
        if (live && l16 == 0) {
            const uint32_t lc = len < RC_REPORT_MAX_LEN - 1 ? len : RC_REPORT_MAX_LEN - 1, key = (mate << 10) | lc;
            if (key != run_key) {
                flush_run();
                run_key = key;
            }
            ++run_n;
            if (tot == 0) {
                ++run_clean;
            } else {
                atomicAdd(&s_bin[RC_REP_CHANGED + mate], 1u);
                atomicAdd(&s_bin[RC_REP_CHANGES + mate], tot);
                atomicAdd(&s_bin[RC_REP_PER_READ + (tot < RC_REPORT_MAX_PER_READ ? tot : RC_REPORT_MAX_PER_READ)], 1u);
            }
            if (rt == -1) atomicAdd(&s_bin[RC_REP_UNFIX + mate], 1u);
        }
        r = rn;
        o = no;
        o1 = no1;
    }
    flush_run();
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < RC_REPORT_WORDS; b += RC_REP_THREADS) {
        const uint32_t v = s_bin[b];
        if (v) atomicAdd(&A.out[b], (unsigned long long)v);
    }
}

// a batch's staged report added to the context's (a packed or resident batch is counted when its wait accepts it)
__global__ __launch_bounds__(256) void k_report_commit(const unsigned long long *__restrict__ staged, unsigned long long *__restrict__ out)
{
    const uint32_t b = blockIdx.x * 256u + threadIdx.x;
    if (b < RC_REPORT_WORDS) {
        const unsigned long long v = staged[b];
        if (v) atomicAdd(&out[b], v);
    }
}

int rc_launch_change_report(rc_ctx *ctx, const rc_device_batch_args &a, const uint8_t *d_snap, unsigned long long *d_out)
{
    if (a.n == 0) return RC_OK;
    rc_report_args A;
    A.seq = a.seq;
    A.snap_delta = d_snap - a.seq;
    A.off = a.off;
    A.ret = a.ret;
    A.qual = a.qual;
    A.qual_bits = a.qual_bits;
    A.qual_split = a.qual_split;
    A.qual_base2 = a.qual_base2;
    A.bad_qual = ctx->P.bad_qual;
    A.mode = a.mode;
    A.n = a.n;
    A.out = d_out;
    // The kernel reads both sides in whole aligned 16-byte pieces: up to 15 bytes in front of a.seq and behind its last read
    // (memory of the caller of rc_correct_device that the library does not own, and bytes of the snapshot buffer nothing
    // has written) are loaded and masked off.  An aligned 16-byte piece that holds one byte of the arena lies in that byte's
    // page, so the loads cannot fault; an allocator or checker that is exact to the byte would have to know.
    if (A.snap_delta & 15) {
        rc_set_error(ctx, "change report: internal: the snapshot does not have the arena's alignment");
        return RC_ERR_STATE;
    }
    // persistent workgroups: four of 512 threads fill a CU's wave slots, and their histograms (25 KB each) its LDS
    unsigned g = (a.n + RC_REP_QUARTERS - 1) / RC_REP_QUARTERS;
    if (g > (unsigned)ctx->n_cu * 4u) g = (unsigned)ctx->n_cu * 4u;
    hipLaunchKernelGGL(k_change_report, dim3(g), dim3(RC_REP_THREADS), 0, ctx->stream, A);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}

int rc_launch_report_commit(rc_ctx *ctx, const unsigned long long *d_staged, unsigned long long *d_out)
{
    hipLaunchKernelGGL(k_report_commit, dim3((RC_REPORT_WORDS + 255) / 256), dim3(256), 0, ctx->stream, d_staged, d_out);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
