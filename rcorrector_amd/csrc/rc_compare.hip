// rc_compare.hip -- two k-mer tables side by side (include/rcorrector_amd.h: rc_table_compare): the joint count matrix of the
// canonical k-mers of tables a and b, and the mass each carries in the k-mers they share.
//
// One kernel, launched twice.  Pass 0 scans a's buckets and probes b with every live entry's key: cell (fold(count a),
// fold(count b)), a's statistics, and the shared ones.  Pass 1 scans b and probes a, and keeps only the k-mers a does not
// hold: row 0 of the matrix; b's distinct / mass / max are taken from all of its live entries on the way.  So every k-mer
// is counted once, whichever tables hold it.
//
// The scan is k_spectrum_table's (rc_table.hip): grid-stride over the buckets, a lane takes whole buckets with two 16-byte
// loads each (a wavefront's load covers 64 consecutive buckets), the slots are decoded in registers, and the live rule is
// rc_table_slot_entry's first match -- decided in registers for an entry that sits in its home bucket (only an earlier slot
// of the same bucket can shadow it), by rc_table_slot_entry itself for a displaced one (a few per cent).  The probe is the
// per-lane rc_table_lookup, compiled for the probed table's ext = 0 and for the general case.
//
// Cells: a workgroup keeps the RC_CMP_CORNER x RC_CMP_CORNER low corner of the matrix in LDS and flushes its non-zero
// words once; cells outside go to the device array.  Either way the lanes of a wavefront that share the FIRST live lane's
// cell are counted by one ballot and added by that lane alone -- a table whose k-mers all fall into one cell then costs one
// atomic per wavefront and slot round instead of up to 64 on one word -- and the others add for themselves.  (DESIGN.md,
// "Two tables side by side", has the reasons for the corner's size, the buckets in flight and the workgroup.)
#include "rc_internal.h"
#include "rc_device.h"
#include "rc_compare.h"

#define RC_CMP_THREADS 256
#define RC_CMP_WAVES (RC_CMP_THREADS / 64)
#define RC_CMP_UNROLL 2  // buckets per lane in flight (two 16-byte loads each)
#define RC_CMP_MAX_BLOCKS 2048

struct rc_cmp_acc {
    uint64_t distinct = 0, shared = 0;            // wave-uniform (ballot counts)
    uint64_t mass = 0, smass = 0, smass_o = 0;    // per lane: scanned counts, those of shared k-mers, the other table's for them
    uint32_t max_count = 0;                       // per lane
};

// one slot round of a wavefront: this lane's entry (live: key, count c >= 1) against the other table.  MUST be called by
// every lane of the wavefront (ballots).  SECOND: pass 1 -- only k-mers the probed table lacks get a cell, (0, fold(c))
template <bool EXT, bool SECOND>
__device__ __forceinline__ void rc_cmp_add(rc_cmp_acc &A, const rc_table_view &O, bool live, uint64_t key, uint32_t c, uint32_t max_bin,
                                           uint32_t *s_corner, unsigned long long *__restrict__ cells)
{
    const uint32_t o = live ? (uint32_t)rc_table_lookup<EXT>(O, key) : 0u;
    A.distinct += (uint64_t)__popcll(__ballot(live));
    if (!SECOND) A.shared += (uint64_t)__popcll(__ballot(live && o != 0));
    if (live) {
        A.mass += c;
        A.max_count = c > A.max_count ? c : A.max_count;
        if (!SECOND && o) {
            A.smass += c;
            A.smass_o += o;
        }
    }
    const bool cell = SECOND ? live && o == 0 : live;
    const uint32_t fc = rc_cmp_fold(c, max_bin), fo = rc_cmp_fold(o, max_bin);
    const uint32_t i = SECOND ? 0u : fc, j = SECOND ? fc : fo;
    const unsigned long long m = __ballot(cell);
    if (!m) return;
    const int leader = __ffsll(m) - 1;
    const uint32_t li = (uint32_t)__shfl((int)i, leader), lj = (uint32_t)__shfl((int)j, leader);
    const bool with_leader = cell && i == li && j == lj;
    const uint32_t n_leader = (uint32_t)__popcll(__ballot(with_leader));
    const bool me = (int)(threadIdx.x & 63) == leader;
    if (cell && (me || !with_leader)) {
        const uint32_t add = me ? n_leader : 1u;
        if (i < RC_CMP_CORNER && j < RC_CMP_CORNER)
            atomicAdd(&s_corner[i * RC_CMP_CORNER + j], add);
        else
            atomicAdd(&cells[(size_t)i * (max_bin + 1) + j], (unsigned long long)add);
    }
}

// T: the scanned table, O: the probed one (same k).  cells: (max_bin + 1)^2 words, then st: RC_CMP_STAT_WORDS words of this pass
template <bool EXT, bool SECOND>
__global__ __launch_bounds__(RC_CMP_THREADS) void k_table_compare(rc_table_view T, rc_table_view O, uint32_t max_bin,
                                                                   unsigned long long *__restrict__ cells, unsigned long long *__restrict__ st)
{
    __shared__ uint32_t s_corner[RC_CMP_CORNER * RC_CMP_CORNER];
    for (uint32_t x = threadIdx.x; x < RC_CMP_CORNER * RC_CMP_CORNER; x += RC_CMP_THREADS) s_corner[x] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    rc_cmp_acc A;
    const size_t nb = T.nbuckets_alloc, per_wave = 64 * RC_CMP_UNROLL;
    const size_t stride = (size_t)gridDim.x * RC_CMP_WAVES * per_wave;
    const uint32_t cmask = RC_PACKED_COUNT_MASK >> T.ext;
    const uint32_t mhi = 0x7FFFFFFFu & ~cmask;  // remainder bits above the count, displacement
    for (size_t base = ((size_t)blockIdx.x * RC_CMP_WAVES + w) * per_wave; base < nb; base += stride) {  // (wave-uniform)
        uint4 v[RC_CMP_UNROLL][2];
#pragma unroll
        for (int u = 0; u < RC_CMP_UNROLL; ++u) {
            const size_t b = base + (size_t)u * 64 + lane;
            v[u][0] = v[u][1] = make_uint4(0, 0, 0, 0);  // (beyond the table: no count in any slot of either layout)
            if (b < nb) {
                const uint4 *p = reinterpret_cast<const uint4 *>(T.buckets + b * RC_BUCKET_DWORDS);
                v[u][0] = p[0];
                v[u][1] = p[1];
            }
        }
#pragma unroll
        for (int u = 0; u < RC_CMP_UNROLL; ++u) {
            const size_t b = base + (size_t)u * 64 + lane;
            const uint32_t d[8] = {v[u][0].x, v[u][0].y, v[u][0].z, v[u][0].w, v[u][1].x, v[u][1].y, v[u][1].z, v[u][1].w};
            if (T.layout) {
#pragma unroll
                for (int s = 0; s < RC_PACKED_SLOTS; ++s) {
                    const uint32_t lo = d[2 * s], hi = d[2 * s + 1];
                    uint32_t c = hi & cmask;
                    bool live = c != 0;
                    uint64_t key = 0;
                    if (live) {
                        const uint32_t disp = (hi >> 27) & 15u;
                        if (disp == 0) {  // in its home bucket, where the walk starts: an earlier slot with the same key wins
#pragma unroll
                            for (int i = 0; i < s; ++i)
                                if ((d[2 * i + 1] & cmask) != 0 && d[2 * i] == lo && ((d[2 * i + 1] ^ hi) & mhi) == 0) live = false;
                            if (live) {
                                key = rc_packed_key((uint32_t)b, lo, (hi & RC_PACKED_COUNT_MASK) >> (27 - T.ext), T.ext, T.k, T.nb_home);
                                if (c == cmask) c = (uint32_t)rc_packed_overflow_count(T, key);  // (rare) the full count lives in the prefix
                            }
                        } else {  // (displaced: the walk from the key's home, in memory)
                            int32_t cc = 0;
                            live = rc_table_slot_entry(T, b, s, &key, &cc);
                            c = (uint32_t)cc;
                        }
                    }
                    rc_cmp_add<EXT, SECOND>(A, O, live, key, c, max_bin, s_corner, cells);
                }
            } else {
#pragma unroll
                for (int s = 0; s < RC_WIDE_SLOTS; ++s) {
                    const uint32_t c = d[3 * s + 2];
                    bool live = c != 0;
                    const uint64_t key = ((uint64_t)d[3 * s + 1] << 32) | d[3 * s];
                    if (live) {
                        if (rc_home(key, T.nb_home) == b) {
#pragma unroll
                            for (int i = 0; i < s; ++i)
                                if (d[3 * i + 2] != 0 && d[3 * i] == d[3 * s] && d[3 * i + 1] == d[3 * s + 1]) live = false;
                        } else {
                            uint64_t kk;
                            int32_t cc;
                            live = rc_table_slot_entry(T, b, s, &kk, &cc);
                        }
                    }
                    rc_cmp_add<EXT, SECOND>(A, O, live, key, c, max_bin, s_corner, cells);
                }
            }
        }
    }
    // the wavefront's statistics: one atomic per quantity that is not zero
    unsigned long long mass = A.mass, smass = A.smass, smass_o = A.smass_o;
    uint32_t mx = A.max_count;
    for (int o = 32; o > 0; o >>= 1) {
        mass += __shfl_xor(mass, o, 64);
        smass += __shfl_xor(smass, o, 64);
        smass_o += __shfl_xor(smass_o, o, 64);
        const uint32_t y = (uint32_t)__shfl_xor((int)mx, o, 64);
        mx = y > mx ? y : mx;
    }
    if (lane == 0 && A.distinct) {
        atomicAdd(&st[RC_CMP_DISTINCT], (unsigned long long)A.distinct);
        atomicAdd(&st[RC_CMP_MASS], mass);
        atomicMax(&st[RC_CMP_MAX], (unsigned long long)mx);
        if (A.shared) {
            atomicAdd(&st[RC_CMP_SHARED], (unsigned long long)A.shared);
            atomicAdd(&st[RC_CMP_SMASS], smass);
            atomicAdd(&st[RC_CMP_SMASS_OTHER], smass_o);
        }
    }
    __syncthreads();
    for (uint32_t x = threadIdx.x; x < RC_CMP_CORNER * RC_CMP_CORNER; x += RC_CMP_THREADS) {
        const uint32_t n = s_corner[x], i = x / RC_CMP_CORNER, j = x % RC_CMP_CORNER;
        if (n) atomicAdd(&cells[(size_t)i * (max_bin + 1) + j], (unsigned long long)n);  // (n != 0: i, j <= max_bin)
    }
}

template <bool SECOND>
static int rc_compare_pass(rc_ctx *run, const rc_ctx *scan, const rc_ctx *probe, uint32_t max_bin, unsigned long long *d_cells, unsigned long long *d_st)
{
    const size_t nb = scan->nb_alloc;
    if (!nb) return RC_OK;
    const size_t per_block = (size_t)RC_CMP_WAVES * 64 * RC_CMP_UNROLL;
    const unsigned G = (unsigned)std::min<size_t>(RC_CMP_MAX_BLOCKS, (nb + per_block - 1) / per_block);
    rc_with_ext(probe->ext, [&](auto ext) {
        hipLaunchKernelGGL((k_table_compare<decltype(ext)::value, SECOND>), dim3(G), dim3(RC_CMP_THREADS), 0, run->stream, rc_view(scan), rc_view(probe),
                           max_bin, d_cells, d_st);
    });
    RC_CHECK_HIP(run, hipGetLastError());
    return RC_OK;
}

int rc_launch_table_compare(rc_ctx *a, const rc_ctx *b, uint32_t max_bin, unsigned long long *d_out)
{
    unsigned long long *d_st = d_out + rc_cmp_cells(max_bin);
    int rc = rc_compare_pass<false>(a, a, b, max_bin, d_out, d_st);
    if (rc == RC_OK) rc = rc_compare_pass<true>(a, b, a, max_bin, d_out, d_st + RC_CMP_STAT_WORDS);
    return rc;
}
