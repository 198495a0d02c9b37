// rc_norm.hip -- normalisation by k-mer depth (include/rcorrector_amd.h: rc_norm_select_device; the contract in rc_norm.h): one
// byte per unit from the rc_read_depth of its mates, and the tally of the outcomes and of the unit depths before and after.
//
// One launch, a thread per unit, the grid striding over the batch.  A thread reads its mates' 16 bytes each as one vector load,
// decides (rc_norm.h) and stores its byte.  The tally never meets global memory unit by unit:
//   outcomes   a ballot and a population count per wavefront and round, kept in a register; once per wavefront into LDS
//   bins       real libraries put most units into a few depths, so the histograms are private to the workgroup in LDS: the bins
//              0 .. RC_NORM_LDS_BINS - 1 and the folding bin max_bin -- the one address of the tail that every deep unit shares --
//              have a 32-bit LDS counter each, for `before` and for `after` (a workgroup sees fewer than 2^32 units)
//   the tail   a bin in between (only with max_bin > RC_NORM_LDS_BINS: 512 KiB of counters for max_bin = 65535 fit no LDS) is
//              the sparse end of a depth distribution.  Its units go to global memory, but a wavefront first gathers the lanes
//              that share a bin -- one 64-bit atomic per distinct bin and wavefront, so even a batch that is all one tail depth
//              costs a sixty-fourth of an atomic per unit
// At the end every workgroup adds its non-zero LDS counters to the tally with 64-bit atomics.
#include "rc_internal.h"
#include "rc_norm.h"

#define RC_NORM_THREADS 256
#define RC_NORM_BLOCKS_PER_CU 8
#define RC_NORM_LDS_BINS 4096
static_assert(2 * (RC_NORM_LDS_BINS + 1) * 4 <= 40 * 1024, "four workgroups' histograms fit a CU's LDS");

typedef unsigned long long rc_u64;

// tally: [0, 4) outcomes, [4, 4 + max_bin + 1) before, then after.  d_depth: n_units entries (mode 0), 2 n_units (modes 1, 2).
__global__ __launch_bounds__(RC_NORM_THREADS) void k_norm_select(const int4 *__restrict__ d_depth, uint32_t n_units, int mode, uint64_t unit_base,
                                                                 uint32_t target, uint32_t min_cov, uint64_t seed, uint32_t max_bin,
                                                                 uint8_t *__restrict__ d_keep, rc_u64 *__restrict__ tally)
{
    __shared__ uint32_t s_bin[2][RC_NORM_LDS_BINS + 1];
    __shared__ uint32_t s_out[4];
    const uint32_t t = threadIdx.x, ln = t & 63u;
    // LDS slot s < nb is bin s, slot nb is bin max_bin
    const uint32_t nb = max_bin < (uint32_t)RC_NORM_LDS_BINS ? max_bin : (uint32_t)RC_NORM_LDS_BINS;
    for (uint32_t s = t; s <= nb; s += RC_NORM_THREADS) s_bin[0][s] = s_bin[1][s] = 0;
    if (t < 4) s_out[t] = 0;
    __syncthreads();
    rc_u64 *before = tally + 4, *after = tally + 4 + (size_t)max_bin + 1;
    uint32_t n_out[4] = {0, 0, 0, 0};  // (the wavefront's: the same in every lane)
    // the rounds are the workgroup's: every lane of a wavefront takes part in its ballots, with or without a unit
    for (uint64_t u0 = (uint64_t)blockIdx.x * RC_NORM_THREADS; u0 < n_units; u0 += (uint64_t)gridDim.x * RC_NORM_THREADS) {
        const uint64_t u = u0 + t;
        const bool live = u < n_units;
        uint32_t depth = 0, outcome = RC_NORM_NOVALID;
        if (live) {
            const int4 a = mode == 2 ? d_depth[2 * u] : d_depth[u];  // (valid, q1, median, q3)
            int4 b = {0, 0, 0, 0};
            if (mode == 1) b = d_depth[(uint64_t)n_units + u];
            if (mode == 2) b = d_depth[2 * u + 1];
            const bool has = rc_norm_unit_depth(a.x, a.z, b.x, b.z, &depth);
            outcome = rc_norm_outcome(has, depth, rc_norm_draw(seed, unit_base + u), target, min_cov);
            d_keep[u] = (uint8_t)outcome;
        }
#pragma unroll
        for (uint32_t o = 0; o < 4; ++o) n_out[o] += (uint32_t)__popcll(__ballot(live && outcome == o));
        const bool counted = live && outcome != RC_NORM_NOVALID, kept = live && outcome == RC_NORM_KEPT;
        const uint32_t bin = rc_norm_bin(depth, max_bin);
        const bool in_lds = bin < nb || bin == max_bin;
        if (counted && in_lds) {
            const uint32_t slot = bin < nb ? bin : nb;
            atomicAdd(&s_bin[0][slot], 1u);
            if (kept) atomicAdd(&s_bin[1][slot], 1u);
        }
        rc_u64 todo = __ballot(counted && !in_lds);
        while (todo) {  // (uniform: one round per distinct tail bin of the wavefront)
            const int lead = __ffsll(todo) - 1;
            const uint32_t b = (uint32_t)__shfl((int)bin, lead, 64);
            const rc_u64 same = __ballot(counted && !in_lds && bin == b), same_kept = __ballot(kept && !in_lds && bin == b);
            if (ln == (uint32_t)lead) {
                atomicAdd(&before[b], (rc_u64)__popcll(same));
                if (same_kept) atomicAdd(&after[b], (rc_u64)__popcll(same_kept));
            }
            todo &= ~same;
        }
    }
    if (ln == 0) {
#pragma unroll
        for (uint32_t o = 0; o < 4; ++o)
            if (n_out[o]) atomicAdd(&s_out[o], n_out[o]);
    }
    __syncthreads();
    if (t < 4 && s_out[t]) atomicAdd(&tally[t], (rc_u64)s_out[t]);
    for (uint32_t s = t; s <= nb; s += RC_NORM_THREADS) {
        const uint32_t b = s < nb ? s : max_bin;
        if (s_bin[0][s]) atomicAdd(&before[b], (rc_u64)s_bin[0][s]);
        if (s_bin[1][s]) atomicAdd(&after[b], (rc_u64)s_bin[1][s]);
    }
}

int rc_launch_norm_select(rc_ctx *ctx, const void *d_depth, uint32_t n_units, int mode, uint64_t unit_base, uint32_t target, uint32_t min_cov, uint64_t seed,
                          uint32_t max_bin, uint8_t *d_keep, uint64_t *d_tally)
{
    if (n_units == 0) return RC_OK;
    static_assert(sizeof(int4) == 16, "rc_read_depth");
    const uint64_t blocks = ((uint64_t)n_units + RC_NORM_THREADS - 1) / RC_NORM_THREADS;
    const uint64_t cap = (uint64_t)std::max(1, ctx->n_cu) * RC_NORM_BLOCKS_PER_CU;
    rc_timer_begin(ctx);
    hipLaunchKernelGGL(k_norm_select, dim3((unsigned)std::min(blocks, cap)), dim3(RC_NORM_THREADS), 0, ctx->stream, (const int4 *)d_depth, n_units, mode,
                       unit_base, target, min_cov, seed, max_bin, d_keep, (rc_u64 *)d_tally);
    rc_timer_end(ctx, RC_T_NORM);
    RC_CHECK_HIP(ctx, hipGetLastError());
    return RC_OK;
}
